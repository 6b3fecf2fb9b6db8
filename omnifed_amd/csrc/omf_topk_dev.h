// omf_topk_dev.h — the device steps the exact tail (omf_topk_exact.hip), the receive kernels (omf_topk_recv.hip), the
// index pack (omf_topk_pack.hip) and the value quantiser (omf_topk_qval.hip) share.
#pragma once
#include <stdint.h>

#include "omf_common.h"
#include "omf_topk_layout.h"

namespace omf {

// The tensor t with koff[t] <= j < koff[t + 1] among [lo, hi] (the full range: [0, nt - 1]): the largest
// t with koff[t] <= j.  A tensor with no values shares its koff with the next one, which is then the
// larger t, so no position falls to an empty tensor.  (The same search finds a 32-index group's tensor
// in the packed wire's goff.)
template <class T>
__device__ __forceinline__ int koff_tensor(const T* koff, int lo, int hi, int64_t j) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)koff[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// A 32-value group's tensor on the packed wires: the largest t with goff[t] <= g (a tensor without groups
// shares its goff with the next one, the larger t), goff staged in LDS (s_goff[kArenaMaxTensors + 1]) when
// it fits, as topk_dec_place stages its koff window.
__device__ __forceinline__ int group_tensor(const uint32_t* __restrict__ goff_g, uint32_t* s_goff, int nt, int64_t g) {
  return nt <= topk_layout::kArenaMaxTensors ? koff_tensor(s_goff, 0, nt - 1, g) : koff_tensor(goff_g, 0, nt - 1, g);
}
__device__ __forceinline__ void stage_goff(const uint32_t* __restrict__ goff_g, uint32_t* s_goff, int nt) {
  if (nt > topk_layout::kArenaMaxTensors) return;  // uniform
  for (int t = threadIdx.x; t <= nt; t += kThreads) s_goff[t] = goff_g[t];
  __syncthreads();
}

}  // namespace omf
