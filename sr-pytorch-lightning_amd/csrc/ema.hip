// Exponential moving average (EMA) of every parameter tensor of a model in ONE launch, and the in-place exchange of the weights
// with their averages.
//
// The shadow weights s of all tensors live in one flat fp32 buffer; the tensors are described by the optimizers' device table
// (srk_adam_slot / srk_adam_block, param_table.h: `g` unused, `state_off` the tensor's offset into the shadow buffer, one tensor per
// block of at most 4096 elements).  torch._foreach_lerp_ packs a few dozen tensors into one launch, so RCAN's ~1,600 parameter
// tensors pay Adam's 45 launches again for the average, and an in-place exchange in torch ops pays them twice more per validation;
// here one grid walks the table.  The weight w = 1 - decay and the update count are read from / kept in DEVICE memory, so a captured
// hipGraph replays the update, counts it, and follows a changed decay without a re-capture.
//
//   UPDATE: s = s + w * (p - s)     (three fp32 roundings, no contraction; w == 1 stores p itself, srk.h)      12 B per parameter
//   SWAP  : (p, s) = (s, p)                                                                                    16 B
//   STORE : s = p      LOAD: p = s                                                                              8 B
// All four are HBM-bound streams over the arrays (p, s) through param_table.h's table_walk; an operation is its read and write masks
// and its element rule.
#include "param_table.h"

namespace {

template <int OP>
__global__ __launch_bounds__(TABLE_NT) void ema_kernel(const srk_ema_args a) {
  constexpr unsigned P = 1, S = 2;
  constexpr unsigned READ = OP == SRK_EMA_LOAD ? S : OP == SRK_EMA_STORE ? P : P | S;
  constexpr unsigned WRITE = OP == SRK_EMA_LOAD ? P : OP == SRK_EMA_SWAP ? P | S : S;
  const TableRange r = table_range(a.slots, a.blocks);
  float w = 0.f;
  if constexpr (OP == SRK_EMA_UPDATE) {
    w = a.weight[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.count[0] = a.count[0] + 1;   // the only writer of the launch
  }
  const bool whole = w == 1.f;                               // decay 0: the average IS the parameter (s + (p - s) can miss it by an ulp)
  auto upd = [&](float (&x)[2], float) {
    float &pv = x[0], &sv = x[1];
    if constexpr (OP == SRK_EMA_UPDATE) { const float t = sv + w * (pv - sv); sv = whole ? pv : t; }
    else if constexpr (OP == SRK_EMA_SWAP) { const float t = pv; pv = sv; sv = t; }
    else if constexpr (OP == SRK_EMA_STORE) sv = pv;
    else pv = sv;
  };
  float* const x[2] = {r.sl.p, a.shadow + r.sl.state_off};
  table_walk<READ, WRITE, false>(x, nullptr, r.e0, r.e1, upd);
}

}  // namespace

extern "C" int srk_ema_step(const srk_ema_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->shadow, "srk_ema_step: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_ema_step: %d blocks, %d tensors", a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->op >= SRK_EMA_UPDATE && a->op <= SRK_EMA_LOAD, "srk_ema_step: op %d", a->op);
  SRK_CHECK_ARG(a->op != SRK_EMA_UPDATE || (a->weight && a->count), "srk_ema_step: UPDATE needs the weight and the count");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)a->nblocks), block(TABLE_NT);
  switch (a->op) {
    case SRK_EMA_UPDATE: hipLaunchKernelGGL(ema_kernel<SRK_EMA_UPDATE>, grid, block, 0, st, *a); break;
    case SRK_EMA_SWAP: hipLaunchKernelGGL(ema_kernel<SRK_EMA_SWAP>, grid, block, 0, st, *a); break;
    case SRK_EMA_STORE: hipLaunchKernelGGL(ema_kernel<SRK_EMA_STORE>, grid, block, 0, st, *a); break;
    default: hipLaunchKernelGGL(ema_kernel<SRK_EMA_LOAD>, grid, block, 0, st, *a); break;
  }
  SRK_LAUNCH_CHECK();
  return 0;
}
