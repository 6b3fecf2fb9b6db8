// omf_topk_enc_dev.h — the device steps and constants of the Top-K encoder's two kernel units (omf_topk_sampled.hip,
// omf_topk_exact.hip), one copy each.  Both use mag_key, tprime, block_scan_incl, Item and kNoZeroFill; the candidate
// collector, the item's sub-chunk prefix and the exact path's key constants have their callers in the exact unit today.
#pragma once
#include "omf_common.h"
#include "omf_plan_layout.h"
#include "omf_topk_layout.h"

namespace omf::topk_enc {
using namespace topk_layout;  // the constants and per-tensor rules shared with the host side

constexpr int kShift = 21;  // key (31 bits) >> 21 -> 10-bit bin (exact path)
constexpr int kV = 16;
static_assert(kSub == (int64_t)kV * kThreads * 4, "a flat item: kV float4 per thread");
// Composite candidate key: index << 39 | tensor << 31 | (2^31 - 1 - |t'|bits).  Candidates are
// emitted in index order within each tensor, so a stable radix sort of the low 39 bits alone
// gives (tensor ascending, |t'| descending, index ascending): 5 digit passes instead of 8.
constexpr int kSortBits = 39;
using Item = omf::plan_layout::Item;  // the plan's flat items (omf_plan_layout.h)

__device__ __forceinline__ uint32_t mag_key(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// Block-wide inclusive prefix sum of one value per thread (NT threads): wave shuffles and one
// exchange of the wave totals through s_w[NT / 64].  Every thread must call it; it begins
// with a barrier, so s_w may be reused from one call to the next.
template <int NT>
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* s_w, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  __syncthreads();
  if (lane == 63) s_w[w] = v;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    const uint32_t x = s_w[i];
    pre += i < w ? x : 0u;
    tot += x;
  }
  total = tot;
  return v + pre;
}

// t' of one element: MODE 0/2: alpha * x ; MODE 1: r + alpha * x (the reference's order).
template <int MODE>
__device__ __forceinline__ float tprime(float x, float r, float alpha) {
  const float t = __fmul_rn(x, alpha);
  return MODE == 1 ? __fadd_rn(r, t) : t;
}

// Append the selected elements of one 8 Ki-element pass of an item to the item's region in
// ascending element order (element idx0 + 1024 k + c of thread t is the pass's element
// 1024 k + 4 t + c): the 8 per-row counts of every thread are block-scanned as 16-bit
// fields, so a stable sort on the key bits above the index keeps index order for equal
// magnitudes (torch's tie order) without sorting the index bits.
struct PassCollector {
  uint32_t* s_wsum;  // 4 x kWaves packed row counts
  __device__ __forceinline__ uint32_t append(const float4 (&v)[8], uint32_t selm, uint64_t* dst,
                                             uint32_t idx0) const {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t pk[4], mine[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // rows 2i, 2i+1: counts 0..4 in 16-bit fields
      pk[i] = (uint32_t)__popc((selm >> (8 * i)) & 0xFu) | ((uint32_t)__popc((selm >> (8 * i + 4)) & 0xFu) << 16);
      mine[i] = pk[i];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {  // wave inclusive scan (fields never carry: <= 256)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t u = __shfl_up(pk[i], o, 64);
        if (lane >= o) pk[i] += u;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s_wsum[4 * wave + i] = pk[i];
    }
    __syncthreads();
    uint32_t wpre[4] = {0, 0, 0, 0}, tot[4] = {0, 0, 0, 0};
#pragma unroll
    for (int w2 = 0; w2 < kWaves; ++w2) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t ws = s_wsum[4 * w2 + i];
        if (w2 < wave) wpre[i] += ws;
        tot[i] += ws;  // fields <= 1024: no carry
      }
    }
    __syncthreads();  // s_wsum reuse by the next pass
    uint32_t rowbase = 0, total = 0;
    uint32_t base[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = k >> 1, sh = 16 * (k & 1);
      const uint32_t ex = ((pk[i] - mine[i]) >> sh) & 0xFFFFu;  // threads before me in my wave
      base[k] = rowbase + ((wpre[i] >> sh) & 0xFFFFu) + ex;
      rowbase += (tot[i] >> sh) & 0xFFFFu;
    }
    total = rowbase;
    if (selm) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float vv[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        uint32_t r = base[k];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if ((selm >> (4 * k + c)) & 1u) {
            const uint32_t idx = idx0 + 1024u * k + c;
            dst[r++] = ((uint64_t)idx << 32) | (uint64_t)__float_as_uint(vv[c]);
          }
        }
      }
    }
    return total;
  }
};

// The kSubsPerItem sub-chunk candidate counts of item `item` -> s_pre[0..32] (exclusive prefix, s_pre[32]
// = the item's total).  Wave 0 scans; ends with a block barrier.
__device__ __forceinline__ void item_prefix(const uint32_t* __restrict__ sub_cnt, int64_t item, uint32_t* s_pre) {
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    uint32_t v = l < kSubsPerItem ? sub_cnt[(size_t)item * kSubsPerItem + l] : 0u;
#pragma unroll
    for (int d = 1; d < kSubsPerItem; d <<= 1) {
      const uint32_t u = __shfl_up(v, d, 64);
      if (l >= d) v += u;
    }
    if (l < kSubsPerItem) s_pre[l + 1] = v;
    if (l == 0) s_pre[0] = 0;
  }
  __syncthreads();
}

// Candidate e of the item (in index order): sub j's run lives at the sub's element range.
__device__ __forceinline__ uint64_t item_key(const uint64_t* __restrict__ cand, int64_t begin, const uint32_t* s_pre,
                                             uint32_t e) {
  int j = 0;  // the sub with s_pre[j] <= e < s_pre[j + 1]
#pragma unroll
  for (int h = kSubsPerItem / 2; h > 0; h >>= 1)
    if (s_pre[j + h] <= e) j += h;
  return cand[begin + (int64_t)j * kSubPer + (e - s_pre[j])];
}

// zcnt[t] of a tensor without a zero fill (topk_plan_tensor writes it, zero_fill_chunk reads it).
constexpr uint32_t kNoZeroFill = 0xffffffffu;

}  // namespace omf::topk_enc
