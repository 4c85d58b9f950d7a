// Gradient accumulation over micro-batches (Lightning's `accumulate_grad_batches`) as launches of the training step.
//
// The running sum `acc` of a window's gradients lives in one flat fp32 buffer per parameter group, laid out like the optimizers' flat
// state (tensor i at `state_off`); the gradients are those of the optimizers' device table (srk_adam_slot / srk_adam_block,
// param_table.h), one workgroup per block of at most 4096 elements of ONE tensor.  `acc` is zero at the start of a window.
//
//   ADD   (micro-steps 1 .. k-1): acc = acc + g                                                   12 B per parameter
//   FINAL (micro-step k)        : g = (acc + g) * inv_k;  acc = 0                                 16 B
// fp32 throughout, two roundings in FINAL, nothing contracted; non-finite values pass through like any other (srk.h).  FINAL leaves
// the averaged gradient where clipping and the optimizers read gradients, and zeroes `acc` itself: no launch tests a "first
// micro-step" flag, so no block reads a counter that another block of the same launch writes.  Which of the two runs is decided on
// the host (by which hipGraph is replayed).  Both are HBM-bound streams over the arrays (acc, g) through param_table.h's table_walk.
#include "param_table.h"

namespace {

template <int OP>
__global__ __launch_bounds__(TABLE_NT) void grad_accum_kernel(const srk_grad_accum_args a) {
  constexpr unsigned ACC = 1, G = 2;
  constexpr unsigned WRITE = OP == SRK_ACCUM_ADD ? ACC : ACC | G;
  const TableRange r = table_range(a.slots, a.blocks);
  const float inv_k = a.inv_k;
  auto upd = [&](float (&x)[2], float) {
    const float s = x[0] + x[1];
    if constexpr (OP == SRK_ACCUM_ADD) x[0] = s;
    else { x[1] = s * inv_k; x[0] = 0.f; }
  };
  float* const x[2] = {a.acc + r.sl.state_off, const_cast<float*>(r.sl.g)};
  table_walk<ACC | G, WRITE, false>(x, nullptr, r.e0, r.e1, upd);
}

}  // namespace

extern "C" int srk_grad_accum(const srk_grad_accum_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->acc, "srk_grad_accum: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_grad_accum: %d blocks, %d tensors", a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->op == SRK_ACCUM_ADD || a->op == SRK_ACCUM_FINAL, "srk_grad_accum: op %d", a->op);
  SRK_CHECK_ARG(a->inv_k > 0.f && a->inv_k <= 1.f, "srk_grad_accum: inv_k %g (1 / k for a window of k >= 1 micro-steps)", (double)a->inv_k);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)a->nblocks), block(TABLE_NT);
  if (a->op == SRK_ACCUM_ADD) hipLaunchKernelGGL(grad_accum_kernel<SRK_ACCUM_ADD>, grid, block, 0, st, *a);
  else hipLaunchKernelGGL(grad_accum_kernel<SRK_ACCUM_FINAL>, grid, block, 0, st, *a);
  SRK_LAUNCH_CHECK();
  return 0;
}
