// Exponential moving average (EMA) of every parameter tensor of a model in ONE launch, and the in-place exchange of the weights
// with their averages.
//
// The shadow weights s of all tensors live in one flat fp32 buffer; the tensors are described by the optimizers' device table
// (srk_adam_slot / srk_adam_block of optim.hip: `g` unused, `state_off` the tensor's offset into the shadow buffer, one tensor per
// block of at most 4096 elements).  torch._foreach_lerp_ packs a few dozen tensors into one launch, so RCAN's ~1,600 parameter
// tensors pay Adam's 45 launches again for the average, and an in-place exchange in torch ops pays them twice more per validation;
// here one grid walks the table.  The weight w = 1 - decay and the update count are read from / kept in DEVICE memory, so a captured
// hipGraph replays the update, counts it, and follows a changed decay without a re-capture.
//
//   UPDATE: s = s + w * (p - s)     (three fp32 roundings, no contraction; w == 1 stores p itself, srk.h)      12 B per parameter
//   SWAP  : (p, s) = (s, p)                                                                                    16 B
//   STORE : s = p      LOAD: p = s                                                                              8 B
// All four are HBM-bound streams with adam_group_kernel's access pattern: 4 x float4 per array and thread with every load issued
// before the first use when the addresses allow 16-byte accesses, a scalar path otherwise, a scalar tail.
#include "srk_common.h"

namespace {

constexpr int EMA_NT = 256;

template <int OP>
__global__ __launch_bounds__(EMA_NT) void ema_kernel(const srk_ema_args a) {
  constexpr bool READ_P = OP != SRK_EMA_LOAD, READ_S = OP == SRK_EMA_UPDATE || OP == SRK_EMA_SWAP || OP == SRK_EMA_LOAD;
  constexpr bool WRITE_P = OP == SRK_EMA_SWAP || OP == SRK_EMA_LOAD, WRITE_S = OP != SRK_EMA_LOAD;
  const srk_adam_block blk = a.blocks[blockIdx.x];
  const srk_adam_slot sl = a.slots[blk.slot];
  float w = 0.f;
  if constexpr (OP == SRK_EMA_UPDATE) {
    w = a.weight[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.count[0] = a.count[0] + 1;   // the only writer of the launch
  }
  const bool whole = w == 1.f;                               // decay 0: the average IS the parameter (s + (p - s) can miss it by an ulp)
  const long long e0 = blk.start, e1 = (e0 + blk.count < sl.n) ? e0 + blk.count : sl.n;
  float* const p = sl.p;
  float* const s = a.shadow + sl.state_off;
  auto upd = [&](float& pv, float& sv) {
    if constexpr (OP == SRK_EMA_UPDATE) { const float t = sv + w * (pv - sv); sv = whole ? pv : t; }
    else if constexpr (OP == SRK_EMA_SWAP) { const float t = pv; pv = sv; sv = t; }
    else if constexpr (OP == SRK_EMA_STORE) sv = pv;
    else pv = sv;
  };
  auto upd1 = [&](long long e) {
    float pv = 0.f, sv = 0.f;
    if constexpr (READ_P) pv = p[e];
    if constexpr (READ_S) sv = s[e];
    upd(pv, sv);
    if constexpr (WRITE_P) p[e] = pv;
    if constexpr (WRITE_S) s[e] = sv;
  };
  // 16-byte accesses when both arrays allow it (tensor starts inside the flat shadow buffer are 4-float aligned; a parameter that
  // is a view into a larger storage need not be)
  const bool vec = (((uintptr_t)p | (uintptr_t)s) & 15) == 0 && (e0 & 3) == 0;
  if (vec) {
    const long long n4 = (e1 - e0) >> 2;
    for (long long i0 = 0; i0 < n4; i0 += 4 * EMA_NT) {
      f32x4 p4[4], s4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * EMA_NT + threadIdx.x;
        p4[u] = s4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n4) {
          const long long e = e0 + 4 * i;
          if constexpr (READ_P) p4[u] = *reinterpret_cast<const f32x4*>(p + e);
          if constexpr (READ_S) s4[u] = *reinterpret_cast<const f32x4*>(s + e);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * EMA_NT + threadIdx.x;
        if (i < n4) {
          const long long e = e0 + 4 * i;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float pv = p4[u][k], sv = s4[u][k];
            upd(pv, sv);
            p4[u][k] = pv; s4[u][k] = sv;
          }
          if constexpr (WRITE_P) *reinterpret_cast<f32x4*>(p + e) = p4[u];
          if constexpr (WRITE_S) *reinterpret_cast<f32x4*>(s + e) = s4[u];
        }
      }
    }
    for (long long e = e0 + 4 * n4 + threadIdx.x; e < e1; e += EMA_NT) upd1(e);
  } else {
    for (long long e = e0 + threadIdx.x; e < e1; e += EMA_NT) upd1(e);
  }
}

}  // namespace

extern "C" int srk_ema_step(const srk_ema_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->shadow, "srk_ema_step: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_ema_step: %d blocks, %d tensors", a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->op >= SRK_EMA_UPDATE && a->op <= SRK_EMA_LOAD, "srk_ema_step: op %d", a->op);
  SRK_CHECK_ARG(a->op != SRK_EMA_UPDATE || (a->weight && a->count), "srk_ema_step: UPDATE needs the weight and the count");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)a->nblocks), block(EMA_NT);
  switch (a->op) {
    case SRK_EMA_UPDATE: hipLaunchKernelGGL(ema_kernel<SRK_EMA_UPDATE>, grid, block, 0, st, *a); break;
    case SRK_EMA_SWAP: hipLaunchKernelGGL(ema_kernel<SRK_EMA_SWAP>, grid, block, 0, st, *a); break;
    case SRK_EMA_STORE: hipLaunchKernelGGL(ema_kernel<SRK_EMA_STORE>, grid, block, 0, st, *a); break;
    default: hipLaunchKernelGGL(ema_kernel<SRK_EMA_LOAD>, grid, block, 0, st, *a); break;
  }
  SRK_LAUNCH_CHECK();
  return 0;
}
