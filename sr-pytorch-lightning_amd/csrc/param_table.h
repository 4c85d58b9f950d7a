// The device table of parameter tensors (srk_adam_slot / srk_adam_block, include/srk.h) and the one walk over it that every table
// kernel shares: the optimizers of optim.hip and the EMA of ema.hip.
//
// A launch has one workgroup of TABLE_NT threads per block of the table; a block is at most 4096 elements of ONE tensor, so every
// per-tensor decision (a step count, "first step", a Lookahead sync) is uniform over the workgroup.  A table kernel supplies
//   - its scalar set-up (hyper-parameters, the tensor's count), formed once per workgroup;
//   - the arrays it walks: N float arrays of the tensor (the parameter and its slices of the flat state buffers) and, optionally,
//     the read-only gradient;
//   - which arrays are read and which are written, as compile-time masks (bit j = array j);
//   - the element rule `upd(x, g)`: x[j] is the element of array j (0.f on entry where array j is not read), g the gradient's;
// and calls table_walk once.  All of them are HBM-bound streams, so the walk is the whole performance story of these kernels.
#pragma once
#include "srk_common.h"

namespace {

constexpr int TABLE_NT = 256;

// block index -> the tensor and its element range [e0, e1)
struct TableRange {
  srk_adam_slot sl;
  long long e0, e1;
};

__device__ __forceinline__ TableRange table_range(const srk_adam_slot* slots, const srk_adam_block* blocks) {
  const srk_adam_block blk = blocks[blockIdx.x];
  TableRange r;
  r.sl = slots[blk.slot];
  r.e0 = blk.start;
  r.e1 = (r.e0 + blk.count < r.sl.n) ? r.e0 + blk.count : r.sl.n;
  return r;
}

// The elements [e0, e1) of N arrays (and of g when GRAD): 16-byte accesses when every address allows it (tensor starts inside the
// flat state buffers are 4-float aligned; a parameter or gradient that is a view into a larger storage need not be), 4 x float4 per
// array and thread with ALL loads issued before the first use (a 4096-element block is one pass), a scalar tail; a scalar path
// otherwise.  Both paths apply the same `upd` to the same values, so they give the same bits.
// READ / WRITE are template arguments, not runtime selects on the loads and stores: an array that a block-uniform decision leaves
// unread (Ranger's slow weights outside a sync step, SGD's momentum buffer at a tensor's first step) is a different instantiation,
// chosen by the caller with a uniform branch.  Conditional 16-byte loads doubled Ranger's register count (210 VGPRs, occupancy 2,
// against 130 / 3 as a template).
template <unsigned READ, unsigned WRITE, bool GRAD, int N, class F>
__device__ __forceinline__ void table_walk(float* const (&arrays)[N], const float* const grad, const long long e0, const long long e1, F upd) {
  // the range's own start and length: a block's count is an int, so everything below indexes with 32 bits from uniform bases
  float* a[N];
#pragma unroll
  for (int j = 0; j < N; ++j) a[j] = arrays[j] + e0;
  const float* const g = GRAD ? grad + e0 : nullptr;
  const int n = (int)(e1 - e0);
  auto upd1 = [&](int e) {
    float x[N] = {}, gv = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (READ >> j & 1) x[j] = a[j][e];
    if constexpr (GRAD) gv = g[e];
    upd(x, gv);
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (WRITE >> j & 1) a[j][e] = x[j];
  };
  uintptr_t bits = (uintptr_t)g;
#pragma unroll
  for (int j = 0; j < N; ++j) bits |= (uintptr_t)a[j];
  if ((bits & 15) == 0) {                    // the range starts 16-byte aligned in every array
    const int n4 = n >> 2;
    for (int i0 = 0; i0 < n4; i0 += 4 * TABLE_NT) {
      f32x4 x4[N][4], g4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * TABLE_NT + threadIdx.x;
        g4[u] = f32x4{0.f, 0.f, 0.f, 0.f};       // (defined on every path: the compiler allocates fewer registers than for an undefined one)
        if (i < n4) {
#pragma unroll
          for (int j = 0; j < N; ++j)
            if (READ >> j & 1) x4[j][u] = *reinterpret_cast<const f32x4*>(a[j] + 4 * i);
          if constexpr (GRAD) g4[u] = *reinterpret_cast<const f32x4*>(g + 4 * i);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * TABLE_NT + threadIdx.x;
        if (i < n4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float x[N];
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = (READ >> j & 1) ? x4[j][u][k] : 0.f;
            upd(x, GRAD ? g4[u][k] : 0.f);
#pragma unroll
            for (int j = 0; j < N; ++j) x4[j][u][k] = x[j];
          }
#pragma unroll
          for (int j = 0; j < N; ++j)
            if (WRITE >> j & 1) *reinterpret_cast<f32x4*>(a[j] + 4 * i) = x4[j][u];
        }
      }
    }
    for (int e = 4 * n4 + threadIdx.x; e < n; e += TABLE_NT) upd1(e);
  } else {
    for (int e = threadIdx.x; e < n; e += TABLE_NT) upd1(e);
  }
}

// The two launches around an update under dynamic loss scaling (`state`: DeviceGradScaler's floats, optim.hip).  They read the
// table and the counts only, so every optimizer launches them as they are.  (Templates over the workgroup size, so that a file that
// includes this header without launching them -- ema.hip -- carries no copy of them.)
//   adam_check_kernel : state[2] (found_inf) = 1 if any gradient of the table is not finite
template <int NT>
__global__ __launch_bounds__(NT) void adam_check_kernel(const srk_adam_slot* __restrict__ slots, const srk_adam_block* __restrict__ blocks,
                                                        float* __restrict__ state) {
  const TableRange r = table_range(slots, blocks);
  bool bad = false;
  for (long long e = r.e0 + threadIdx.x; e < r.e1; e += NT) bad |= !isfinite(r.sl.g[e]);
  if (bad) state[2] = 1.f;                  // every writer stores the same value
}

//   adam_bump_kernel  : the second launch of a step: the update has read every count, advance the counts of the tensors in the
// table -- unless the step is skipped (`state` may be NULL: no loss scaling).  (A "last block bumps" ticket inside the update costs
// one same-address atomic per block: 5k blocks serialise to 0.3 ms.)
template <int NT>
__global__ __launch_bounds__(NT) void adam_bump_kernel(const srk_adam_slot* __restrict__ slots, int nslots, float* __restrict__ steps,
                                                       const float* __restrict__ state) {
  if (state && state[2] != 0.f) return;
  for (int i = blockIdx.x * NT + threadIdx.x; i < nslots; i += gridDim.x * NT) steps[slots[i].step_idx] += 1.f;
}

}  // namespace
