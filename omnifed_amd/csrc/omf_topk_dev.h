// omf_topk_dev.h — the device step the exact tail (omf_topk.hip), the receive kernels (omf_topk_recv.hip) and
// the index pack (omf_topk_pack.hip) share.
#pragma once
#include <stdint.h>

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

}  // namespace omf
