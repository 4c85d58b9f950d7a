// Learning-rate schedules whose state lives on the DEVICE: one step count and one double per parameter group, advanced by ONE tiny
// launch behind every optimizer step.
//
// The optimizers take `lr` by value in their launch arguments, so a captured hipGraph replays the learning rate it was captured
// with, and a per-iteration schedule would re-capture every step.  Their `lr_dev` (srk.h) reads ONE device double when the launch
// runs instead; this kernel is what writes it.  Captured behind the step it belongs to (SRK_LR_ADVANCE), every replay counts itself
// and leaves the next step's learning rate behind.
//
//   f(t, base) = warm(t) * main(t, base)            torch.optim.lr_scheduler's closed forms (srk.h has the table), all in double
// One workgroup of one wave; thread g owns group g (a loop over the groups beyond 64).  Every thread reads the count, thread 0 is
// its only writer (an ordinary store behind a barrier).  The restart schedule finds (T_cur, T_i) by the integer loop, not by a
// logarithm: at a restart boundary a logarithm that is one ulp short picks the wrong cycle.
#include "srk_common.h"

namespace {

constexpr int LR_NT = 64;

// the launch's constants: srk_lr_sched_args with the milestones as an array
struct LrSched {
  long long* count; double* lr; const double* base_lr; int ngroups;
  int kind, op;
  long long value, step_size, t_max, t_0, t_mult, warmup_steps;
  double gamma, eta_min, warmup_start;
  int nmilestones;
  long long milestones[SRK_LR_MAX_MILESTONES];
};

__device__ __forceinline__ double half_cosine(double base, double eta_min, long long num, long long den) {
  const double pi = 3.141592653589793;       // math.pi
  return eta_min + (base - eta_min) * (1.0 + cos(pi * (double)num / (double)den)) / 2.0;
}

__global__ __launch_bounds__(LR_NT) void lr_sched_kernel(const LrSched s) {
  const long long t = s.op == SRK_LR_SET ? s.value : s.count[0] + 1;
  __syncthreads();                           // every thread has read the count
  if (threadIdx.x == 0) s.count[0] = t;
  double warm = 1.0;
  if (s.warmup_steps > 0) {
    const long long tw = t < s.warmup_steps ? t : s.warmup_steps;
    warm = s.warmup_start + (1.0 - s.warmup_start) * (double)tw / (double)s.warmup_steps;
  }
  // what does not depend on the group
  double decay = 1.0;                        // STEP, MULTISTEP: gamma^n
  long long num = 0, den = 1;                // COSINE*: the phase num / den
  if (s.kind == SRK_LR_STEP) {
    decay = pow(s.gamma, (double)(t / s.step_size));
  } else if (s.kind == SRK_LR_MULTISTEP) {
    int n = 0;
    for (int i = 0; i < SRK_LR_MAX_MILESTONES; ++i) n += (i < s.nmilestones && s.milestones[i] <= t) ? 1 : 0;
    decay = pow(s.gamma, (double)n);
  } else if (s.kind == SRK_LR_COSINE) {
    num = t; den = s.t_max;
  } else if (s.kind == SRK_LR_COSINE_RESTARTS) {
    num = t; den = s.t_0;
    if (s.t_mult == 1) {
      num = t % s.t_0;                       // the loop's result without its t / t_0 iterations
    } else {
      while (num >= den) { num -= den; den *= s.t_mult; }       // at most log2(t / t_0) + 1 iterations
    }
  }
  for (int g = threadIdx.x; g < s.ngroups; g += LR_NT) {
    const double base = s.base_lr[g];
    double v;
    if (s.kind == SRK_LR_STEP || s.kind == SRK_LR_MULTISTEP) v = base * decay;
    else if (s.kind == SRK_LR_COSINE || s.kind == SRK_LR_COSINE_RESTARTS) v = half_cosine(base, s.eta_min, num, den);
    else v = base;
    s.lr[g] = warm * v;
  }
}

}  // namespace

extern "C" int srk_lr_sched_step(const srk_lr_sched_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->count && a->lr && a->base_lr, "srk_lr_sched_step: null pointer");
  SRK_CHECK_ARG(a->ngroups > 0, "srk_lr_sched_step: %d groups", a->ngroups);
  SRK_CHECK_ARG(a->kind >= SRK_LR_CONSTANT && a->kind <= SRK_LR_COSINE_RESTARTS, "srk_lr_sched_step: kind %d", a->kind);
  SRK_CHECK_ARG(a->op == SRK_LR_SET || a->op == SRK_LR_ADVANCE, "srk_lr_sched_step: op %d", a->op);
  SRK_CHECK_ARG(a->op != SRK_LR_SET || a->value >= 0, "srk_lr_sched_step: SET to count %lld", a->value);
  SRK_CHECK_ARG(a->warmup_steps >= 0 && a->warmup_start > 0.0 && a->warmup_start <= 1.0,
                "srk_lr_sched_step: warmup_steps=%lld warmup_start=%g (0 < warmup_start <= 1)", a->warmup_steps, a->warmup_start);
  LrSched s = {};
  s.count = a->count; s.lr = a->lr; s.base_lr = a->base_lr; s.ngroups = a->ngroups;
  s.kind = a->kind; s.op = a->op; s.value = a->value;
  s.warmup_steps = a->warmup_steps; s.warmup_start = a->warmup_start;
  s.step_size = s.t_max = s.t_0 = s.t_mult = 1;
  switch (a->kind) {
    case SRK_LR_STEP:
      SRK_CHECK_ARG(a->step_size >= 1, "srk_lr_sched_step: step_size=%lld", a->step_size);
      s.step_size = a->step_size; s.gamma = a->gamma;
      break;
    case SRK_LR_MULTISTEP: {
      SRK_CHECK_ARG(a->nmilestones >= 0 && a->nmilestones <= SRK_LR_MAX_MILESTONES, "srk_lr_sched_step: %d milestones (at most %d)",
                    a->nmilestones, SRK_LR_MAX_MILESTONES);
      const long long ms[SRK_LR_MAX_MILESTONES] = {a->m0, a->m1, a->m2,  a->m3,  a->m4,  a->m5,  a->m6,  a->m7,
                                                   a->m8, a->m9, a->m10, a->m11, a->m12, a->m13, a->m14, a->m15};
      for (int i = 0; i < a->nmilestones; ++i) {
        SRK_CHECK_ARG(i == 0 || ms[i - 1] <= ms[i], "srk_lr_sched_step: milestones not sorted (%lld before %lld)", ms[i - 1], ms[i]);
        s.milestones[i] = ms[i];
      }
      s.nmilestones = a->nmilestones; s.gamma = a->gamma;
      break;
    }
    case SRK_LR_COSINE:
      SRK_CHECK_ARG(a->t_max >= 1, "srk_lr_sched_step: t_max=%lld", a->t_max);
      s.t_max = a->t_max; s.eta_min = a->eta_min;
      break;
    case SRK_LR_COSINE_RESTARTS:
      SRK_CHECK_ARG(a->t_0 >= 1 && a->t_mult >= 1, "srk_lr_sched_step: t_0=%lld t_mult=%lld", a->t_0, a->t_mult);
      s.t_0 = a->t_0; s.t_mult = a->t_mult; s.eta_min = a->eta_min;
      break;
    default: break;
  }
  hipLaunchKernelGGL(lr_sched_kernel, dim3(1), dim3(LR_NT), 0, reinterpret_cast<hipStream_t>(stream), s);
  SRK_LAUNCH_CHECK();
  return 0;
}
