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
//
// Every kernel here is a table kernel (param_table.h): scalar set-up, element rule, one table_walk.
#include "param_table.h"

namespace {

// Dynamic loss scaling on the DEVICE (fp16 training, the reference's `precision: 16` = Lightning's "16-mixed": autocast +
// torch.amp.GradScaler, configs/all.yml:122): state = {scale, growth tracker, found_inf, growth factor, backoff factor, growth
// interval, skipped steps}.  GradScaler reads found_inf on the HOST every step (`optimizer.step` is skipped from Python), which a
// hipGraph replay cannot do; here the check, the skip and the scale update are launches of the captured step:
//   adam_check_kernel  : found_inf = any gradient not finite           (the gradients are still multiplied by `scale`)
//   adam_group_kernel  : found_inf ? nothing : the update on g / scale
//   adam_bump_kernel   : found_inf ? nothing : step counts += 1
//   scaler_update      : found_inf ? (scale *= backoff, tracker = 0) : (++tracker == interval ? scale *= growth, tracker = 0); found_inf = 0
// -- torch.amp.GradScaler.step / update, same constants, same order.
// (adam_check_kernel and adam_bump_kernel read the table only: param_table.h.)
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
__global__ __launch_bounds__(TABLE_NT) void adam_group_kernel(const srk_adam_args a, const float* __restrict__ state) {
  float inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    inv_scale = 1.f / state[0];
  }
  const TableRange r = table_range(a.slots, a.blocks);
  const srk_adam_slot& sl = r.sl;
  const float t = a.steps[sl.step_idx] + 1.f;
  const float bc1 = 1.f - powf(a.beta1, t), bc2 = 1.f - powf(a.beta2, t);
  const float lr = a.lr_dev ? (float)a.lr_dev[0] : a.lr;    // block-uniform: one scalar load when the launch runs (srk.h `lr_dev`)
  const float step_size = lr / bc1, bc2s = sqrtf(bc2);
  const float b2 = a.beta2, eps = a.eps, wd = a.weight_decay, omb1 = a.one_minus_beta1, omb2 = a.one_minus_beta2;
  auto upd = [&](float (&x)[3], float gv) {
    float &pv = x[0], &mv = x[1], &vv = x[2];
    if constexpr (SCALED) gv *= inv_scale;
    if (a.maximize) gv = -gv;
    if (wd != 0.f) gv += wd * pv;
    mv = mv + (gv - mv) * omb1;                             // torch: exp_avg.lerp_(grad, 1 - beta1)
    vv = b2 * vv + omb2 * gv * gv;                          //        exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(vv) / bc2s + eps;
    pv -= step_size * (mv / denom);
  };
  float* const x[3] = {sl.p, a.m + sl.state_off, a.v + sl.state_off};
  table_walk<7, 7, true>(x, sl.g, r.e0, r.e1, upd);
}


// ---- Ranger (torch_optimizer 0.3.0 `Ranger` = RAdam + Lookahead) over the same table ---------------------------------------
// Per tensor, t = its step count after this step (srk.h has the rule).  The branches -- rectified or not (N_sma > threshold) and
// the Lookahead sync (t % k == 0) -- are decided HERE from the device count, so a replayed hipGraph takes the branch of the
// step it replays, not the one of the step it was captured at.  N_sma and the step size are formed in DOUBLE from double
// hyper-parameters (N_sma cancels: 1999 - 1993.0 at t = 6, so fp32 scalars are off by 0.57 %), then -s*lr is rounded to fp32
// once, as torch rounds a Python scalar; the per-element arithmetic is fp32 in the package's order.
// Traffic: p, m, v read + written, g read = 28 B per parameter; a sync step adds the slow buffer (36 B).  Both branches are
// uniform per block (one tensor per block), so the slow buffer is touched only on sync steps and at t = 1 (slow = p).
// (launch bounds: the waves per SIMD the kernel is allocated for.  Without them the scheduler lets the unscaled form, whose five
// streams leave it 4 registers over the 128 of four waves, drop to three; the scaled form does not fit four without spilling.)
template <bool SCALED>
__global__ __launch_bounds__(TABLE_NT, SCALED ? 3 : 4) void ranger_group_kernel(const srk_ranger_args a, const float* __restrict__ state) {
  // the block-uniform decisions and scalars of the element rule
  struct {
    float inv_scale, step, decay, b1, b2, omb1, omb2, eps, alpha;
    bool wd, rect, sync, first;
  } b;
  b.inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    b.inv_scale = 1.f / state[0];
  }
  const TableRange r = table_range(a.slots, a.blocks);
  const srk_adam_slot& sl = r.sl;
  const long long t = (long long)a.steps[sl.step_idx] + 1;
  const double td = (double)t, b2t = pow(a.beta2, td);
  const double n_max = 2.0 / (1.0 - a.beta2) - 1.0;
  const double n_sma = n_max - 2.0 * td * b2t / (1.0 - b2t);
  b.rect = n_sma > a.n_sma_threshold;
  const double s = b.rect ? sqrt((1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) / (1.0 - pow(a.beta1, td))
                          : 1.0 / (1.0 - pow(a.beta1, td));
  const double lr = a.lr_dev ? a.lr_dev[0] : a.lr;          // block-uniform: one scalar load when the launch runs (srk.h `lr_dev`)
  b.step = (float)(-s * lr);
  b.decay = (float)(-a.weight_decay * lr);
  b.b1 = (float)a.beta1; b.b2 = (float)a.beta2;
  b.omb1 = (float)(1.0 - a.beta1); b.omb2 = (float)(1.0 - a.beta2);
  b.eps = (float)a.eps; b.alpha = (float)a.alpha;
  b.wd = a.weight_decay != 0.0; b.sync = t % a.k == 0; b.first = t == 1;
  // sv: the slow weight on entry (when it is read), written back on a sync step and at the first.  Selects, not branches: the
  // flags are block-uniform
  auto upd = [&](float (&x)[4], float gv) {
    float &pv = x[0], &mv = x[1], &vv = x[2], &sv = x[3];
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
  float* const x[4] = {sl.p, a.m + sl.state_off, a.v + sl.state_off, a.slow + sl.state_off};
  // the slow weights are read on a sync step after the first, written on every sync step and at the first, untouched otherwise
  if (b.sync && !b.first) table_walk<15, 15, true>(x, sl.g, r.e0, r.e1, upd);
  else if (b.first) table_walk<7, 15, true>(x, sl.g, r.e0, r.e1, upd);
  else table_walk<7, 7, true>(x, sl.g, r.e0, r.e1, upd);
}


// ---- SGD and RMSprop (torch.optim.SGD / torch.optim.RMSprop) over the same table ---------------------------------------------
// The models' `optimizer="SGD"` / `"RMSprop"` (reference models/srmodel.py:57-64).  torch's foreach step packs a few dozen tensors
// per launch and makes one pass per _foreach_* op: for RCAN's ~1,600 tensors that is Adam's launch storm once per pass.  Here:
// one launch over Adam's table, one tensor per block, so every per-tensor decision is block-uniform.  srk.h has the rules; the
// element arithmetic is fp32 in the order of torch's _single_tensor_sgd / _single_tensor_rmsprop, and every scalar (-lr,
// 1 - dampening, 1 - alpha) is formed in double and rounded to fp32 once, as torch rounds a Python scalar.
// Only the state a configuration uses is touched: SGD 12 B per parameter (p read + written, g read), 20 B with momentum;
// RMSprop 20 B (square_avg too), +8 B with momentum, +8 B centered.

// torch.optim.SGD.  "first" -- torch creates momentum_buffer as a clone of the first gradient a tensor ever receives, whatever
// `dampening` says -- is read from the tensor's DEVICE count, so a replayed hipGraph gives a tensor whose first gradient arrives
// at a later step the right branch, and a step skipped under loss scaling leaves the tensor "first".
// (launch bounds: allocated for seven waves per SIMD, 72 registers, which the momentum forms otherwise miss by two.)
template <bool SCALED, bool MOM>
__global__ __launch_bounds__(TABLE_NT, 7) void sgd_group_kernel(const srk_sgd_args a, const float* __restrict__ state) {
  float inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    inv_scale = 1.f / state[0];
  }
  constexpr int N = MOM ? 2 : 1;             // p, [momentum_buffer]
  const TableRange r = table_range(a.slots, a.blocks);
  const srk_adam_slot& sl = r.sl;
  const float mom = (float)a.momentum, omd = (float)(1.0 - a.dampening);
  const float wd = (float)a.weight_decay, nlr = (float)(-(a.lr_dev ? a.lr_dev[0] : a.lr));   // (srk.h `lr_dev`: a scalar load)
  const bool has_wd = a.weight_decay != 0.0, nesterov = a.nesterov != 0, maximize = a.maximize != 0;
  bool first = false;
  if constexpr (MOM) first = a.steps[sl.step_idx] == 0.f;
  auto upd = [&](float (&x)[N], float gv) {
    float& pv = x[0];
    float* const sv = x + 1;
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
    float* const x[2] = {sl.p, a.buf + sl.state_off};
    if (first) table_walk<1, 3, true>(x, sl.g, r.e0, r.e1, upd);     // the buffer is written without being read
    else table_walk<3, 3, true>(x, sl.g, r.e0, r.e1, upd);
  } else {
    float* const x[1] = {sl.p};
    table_walk<1, 1, true>(x, sl.g, r.e0, r.e1, upd);
  }
}

// torch.optim.RMSprop.  State arrays in the order square_avg, [momentum_buffer], [grad_avg].
template <bool SCALED, bool MOM, bool CENTERED>
__global__ __launch_bounds__(TABLE_NT) void rmsprop_group_kernel(const srk_rmsprop_args a, const float* __restrict__ state) {
  float inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    inv_scale = 1.f / state[0];
  }
  constexpr int NS = 1 + (MOM ? 1 : 0) + (CENTERED ? 1 : 0);
  const TableRange r = table_range(a.slots, a.blocks);
  const srk_adam_slot& sl = r.sl;
  const float alpha = (float)a.alpha, oma = (float)(1.0 - a.alpha), eps = (float)a.eps;
  const float mom = (float)a.momentum;
  const float wd = (float)a.weight_decay, nlr = (float)(-(a.lr_dev ? a.lr_dev[0] : a.lr));   // (srk.h `lr_dev`: a scalar load)
  const bool has_wd = a.weight_decay != 0.0, maximize = a.maximize != 0;
  const bool lerp_low = oma < 0.5f;          // at::lerp's two forms
  const float omw = 1.f - oma;
  auto upd = [&](float (&x)[NS + 1], float gv) {
    float& pv = x[0];
    float* const sv = x + 1;
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
  float* x[NS + 1];
  x[0] = sl.p;
  x[1] = a.sq + sl.state_off;
  if constexpr (MOM) x[2] = a.buf + sl.state_off;
  if constexpr (CENTERED) x[NS] = a.ga + sl.state_off;
  float* const (&xc)[NS + 1] = x;
  table_walk<(2u << NS) - 1, (2u << NS) - 1, true>(xc, sl.g, r.e0, r.e1, upd);
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
// <name>_check_args refuses bad arguments in the name of the entry point `fn` (the by-value `lr` only when no `lr_dev` replaces it); <name>_launch is the update and, where the optimizer
// keeps counts, the bump (`scaler_state` NULL: no loss scaling).
template <class ARGS>
void check_launch(const ARGS* a, float* scaler_state, hipStream_t st) {
  hipLaunchKernelGGL(adam_check_kernel<TABLE_NT>, dim3((unsigned)a->nblocks), dim3(TABLE_NT), 0, st, a->slots, a->blocks, scaler_state);
}

template <class ARGS>
void bump_launch(const ARGS* a, const float* scaler_state, hipStream_t st) {
  hipLaunchKernelGGL(adam_bump_kernel<TABLE_NT>, dim3((unsigned)((a->nslots + TABLE_NT - 1) / TABLE_NT)), dim3(TABLE_NT), 0, st, a->slots, a->nslots,
                     a->steps, scaler_state);
}

int adam_check_args(const srk_adam_args* a, const char* fn) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->m && a->v && a->steps, "%s: null pointer", fn);
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "%s: %d blocks, %d tensors", fn, a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f && (a->lr_dev || a->lr >= 0.f),
                "%s: lr=%g betas=(%g, %g) eps=%g", fn, a->lr, a->beta1, a->beta2, a->eps);
  return 0;
}

void adam_launch(const srk_adam_args* a, const float* scaler_state, hipStream_t st) {
  const dim3 grid((unsigned)a->nblocks), block(TABLE_NT);
  if (scaler_state) hipLaunchKernelGGL(adam_group_kernel<true>, grid, block, 0, st, *a, scaler_state);
  else hipLaunchKernelGGL(adam_group_kernel<false>, grid, block, 0, st, *a, scaler_state);
  bump_launch(a, scaler_state, st);
}

int ranger_check_args(const srk_ranger_args* a, const char* fn) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->m && a->v && a->slow && a->steps, "%s: null pointer", fn);
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "%s: %d blocks, %d tensors", fn, a->nblocks, a->nslots);
  SRK_CHECK_ARG((a->lr_dev || a->lr > 0.0) && a->alpha >= 0.0 && a->alpha <= 1.0 && a->k >= 1 && a->beta1 >= 0.0 && a->beta1 < 1.0 &&
                a->beta2 >= 0.0 && a->beta2 < 1.0 && a->eps >= 0.0 && a->weight_decay >= 0.0,
                "%s: lr=%g alpha=%g k=%d betas=(%g, %g) eps=%g weight_decay=%g", fn, a->lr, a->alpha, a->k, a->beta1, a->beta2,
                a->eps, a->weight_decay);
  return 0;
}

void ranger_launch(const srk_ranger_args* a, const float* scaler_state, hipStream_t st) {
  const dim3 grid((unsigned)a->nblocks), block(TABLE_NT);
  if (scaler_state) hipLaunchKernelGGL(ranger_group_kernel<true>, grid, block, 0, st, *a, scaler_state);
  else hipLaunchKernelGGL(ranger_group_kernel<false>, grid, block, 0, st, *a, scaler_state);
  bump_launch(a, scaler_state, st);
}

int sgd_check_args(const srk_sgd_args* a, const char* fn) {
  SRK_CHECK_ARG(a && a->slots && a->blocks, "%s: null table", fn);
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "%s: %d blocks, %d tensors", fn, a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->momentum == 0.0 || (a->buf && a->steps), "%s: momentum=%g needs the momentum buffer and the counts", fn, a->momentum);
  SRK_CHECK_ARG((a->lr_dev || a->lr >= 0.0) && a->momentum >= 0.0 && a->weight_decay >= 0.0 && (!a->nesterov || (a->momentum > 0.0 && a->dampening == 0.0)),
                "%s: lr=%g momentum=%g dampening=%g weight_decay=%g nesterov=%d", fn, a->lr, a->momentum, a->dampening, a->weight_decay, a->nesterov);
  return 0;
}

// momentum == 0: no count is kept (nothing is "first"), so the update is the only launch
void sgd_launch(const srk_sgd_args* a, const float* scaler_state, hipStream_t st) {
  const dim3 grid((unsigned)a->nblocks), block(TABLE_NT);
  const bool mom = a->momentum != 0.0;
  if (scaler_state) {
    if (mom) hipLaunchKernelGGL((sgd_group_kernel<true, true>), grid, block, 0, st, *a, scaler_state);
    else hipLaunchKernelGGL((sgd_group_kernel<true, false>), grid, block, 0, st, *a, scaler_state);
  } else {
    if (mom) hipLaunchKernelGGL((sgd_group_kernel<false, true>), grid, block, 0, st, *a, scaler_state);
    else hipLaunchKernelGGL((sgd_group_kernel<false, false>), grid, block, 0, st, *a, scaler_state);
  }
  if (mom) bump_launch(a, scaler_state, st);
}

int rmsprop_check_args(const srk_rmsprop_args* a, const char* fn) {
  SRK_CHECK_ARG(a && a->slots && a->blocks, "%s: null table", fn);
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "%s: %d blocks, %d tensors", fn, a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->sq && a->steps && (a->momentum <= 0.0 || a->buf) && (!a->centered || a->ga), "%s: null state pointer", fn);
  SRK_CHECK_ARG((a->lr_dev || a->lr >= 0.0) && a->alpha >= 0.0 && a->eps >= 0.0 && a->momentum >= 0.0 && a->weight_decay >= 0.0,
                "%s: lr=%g alpha=%g eps=%g momentum=%g weight_decay=%g", fn, a->lr, a->alpha, a->eps, a->momentum, a->weight_decay);
  return 0;
}

template <bool SCALED>
void rmsprop_launch_as(const srk_rmsprop_args* a, const float* scaler_state, hipStream_t st) {
  const dim3 grid((unsigned)a->nblocks), block(TABLE_NT);
  const bool mom = a->momentum > 0.0, cen = a->centered != 0;
  if (mom && cen) hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, true, true>), grid, block, 0, st, *a, scaler_state);
  else if (mom) hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, true, false>), grid, block, 0, st, *a, scaler_state);
  else if (cen) hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, false, true>), grid, block, 0, st, *a, scaler_state);
  else hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, false, false>), grid, block, 0, st, *a, scaler_state);
}

void rmsprop_launch(const srk_rmsprop_args* a, const float* scaler_state, hipStream_t st) {
  if (scaler_state) rmsprop_launch_as<true>(a, scaler_state, st);
  else rmsprop_launch_as<false>(a, scaler_state, st);
  bump_launch(a, scaler_state, st);
}
}  // namespace

// The four entry points of an optimizer: one group; one group under loss scaling; and the two halves of that for optimizers with
// SEVERAL parameter groups: GradScaler.step unscales and checks EVERY group before any is updated -- an inf in group 1
// must not leave group 0 already stepped -- so <name>_check_scaled runs over all groups first, then <name>_update_scaled per group.
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
    check_launch(a, scaler_state, st);                                                                                 \
    NAME##_launch(a, scaler_state, st);                                                                                \
    SRK_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                          \
  }                                                                                                                    \
  extern "C" int srk_##NAME##_check_scaled(const ARGS* a, float* scaler_state, srk_stream_t stream) {                  \
    SRK_CHECK_ARG(a && a->slots && a->blocks && scaler_state, "srk_" #NAME "_check_scaled: null pointer");             \
    SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_" #NAME "_check_scaled: %d blocks, %d tensors", a->nblocks, a->nslots); \
    check_launch(a, scaler_state, reinterpret_cast<hipStream_t>(stream));                                              \
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

SRK_TABLE_STEP_ENTRIES(adam, srk_adam_args)
SRK_TABLE_STEP_ENTRIES(ranger, srk_ranger_args)
SRK_TABLE_STEP_ENTRIES(sgd, srk_sgd_args)
SRK_TABLE_STEP_ENTRIES(rmsprop, srk_rmsprop_args)
#undef SRK_TABLE_STEP_ENTRIES

/* after the LAST parameter group's step of a step under loss scaling: the scale / growth-tracker update (one thread) */
extern "C" int srk_loss_scale_update(float* scaler_state, srk_stream_t stream) {
  SRK_CHECK_ARG(scaler_state, "srk_loss_scale_update: null pointer");
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), scaler_state);
  SRK_LAUNCH_CHECK();
  return 0;
}
