// omf_topk_exact.hip — the Top-K encoder's exact path and the sampled path's device-decided exact tail,
// MI355X (gfx950): their kernels and launches (topk_launch_tail, topk_launch_exact, omf_topk_enc.h), and the
// only use of rocPRIM in the library.  Semantics and the host side: omf_topk.hip.
// Kernel map:
//   the exact path (plans of more than 256 tensors or a tensor over 2^25 elements): topk_prep_hist (t',
//     stored in the EF modes, and its 1024-bin histogram per tensor), topk_select_bin (the k-th magnitude's
//     bin), topk_collect (every t' at or above it as |t'|bits << 32 | ~index), topk_segments and
//     rocprim::segmented_radix_sort_keys_desc (a descending sort per tensor), topk_gather;
//   topk_exact_tail, always enqueued behind the sampled path's groups (no host wait: the call is stream-
//     asynchronous): the zero fill, or on a fallback verdict the exact path behind grid barriers (below).
#include <cstring>  // (rocPRIM's headers use memset)
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <mutex>

#include "omf_topk_dev.h"      // the search over koff shared with the receive kernels
#include "omf_topk_enc.h"      // the plan, the layout, the launchers' declarations
#include "omf_topk_enc_dev.h"  // the device steps shared with omf_topk_sampled.hip

using namespace omf;
using namespace omf::topk_layout;  // the constants and per-tensor rules shared with the host side
using namespace omf::topk_enc;

namespace {

// Exact tail, one block (kThreads): exclusive scan of the per-item candidate counts (items in
// tensor order) in tiles of 1 Ki items (coalesced loads, an LDS scan, a running carry), then per
// tensor its candidate count and start; flag the tensors whose threshold was too high.
// out[0] = all candidates, out[1] = any flagged (agent-scope stores: other blocks read them
// after the tail's grid barrier).
__device__ void scan_check_block(int32_t nt, const int64_t* __restrict__ kk, const uint32_t* __restrict__ tfirst,
                                 const uint32_t* __restrict__ tlast, const uint32_t* __restrict__ item_cnt,
                                 uint32_t* __restrict__ item_off, int64_t n_items, int64_t* __restrict__ cstart,
                                 uint32_t* __restrict__ cnt, uint32_t* __restrict__ flag, uint32_t* out) {
  __shared__ uint32_t part[kWaves];
  __shared__ uint32_t s_any;
  const int t = threadIdx.x;
  if (t == 0) s_any = 0;
  uint32_t carry = 0;
  for (int64_t t0 = 0; t0 < n_items; t0 += 4 * kThreads) {
    uint32_t c[4], loc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // items t0 + 4t + j
      const int64_t i = t0 + 4 * t + j;
      c[j] = i < n_items ? item_cnt[i] : 0u;
      loc += c[j];
    }
    uint32_t tot;
    const uint32_t inc = block_scan_incl<kThreads>(loc, part, tot);
    uint32_t run = carry + inc - loc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = t0 + 4 * t + j;
      if (i < n_items) item_off[i] = run;
      run += c[j];
    }
    carry += tot;
  }
  __threadfence_block();
  __syncthreads();  // item_off of every item visible to the block
  for (int32_t q = t; q < nt; q += kThreads) {
    const uint32_t f = tfirst[q], l = tlast[q];
    const uint32_t of = item_off[f];
    const uint32_t c = item_off[l] + item_cnt[l] - of;
    cstart[q] = of;
    cnt[q] = c;
    const uint32_t redo = (int64_t)c < kk[q] ? 1u : 0u;
    flag[q] = redo;
    if (redo) s_any = 1u;
  }
  __syncthreads();
  if (t == 0) {
    __hip_atomic_store(&out[0], carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&out[1], s_any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Exact path, pass 1 (and the per-tensor redo): t' and its 1024-bin histogram per tensor.
// MODE as topk_fused.  flag != null: only the flagged tensors (a redo reads t' as x with
// MODE 0 and alpha = the scale of t').
template <int MODE>
__device__ void prep_hist_item(const float* __restrict__ x, float* __restrict__ r, float alpha,
                               const Item* __restrict__ items, const uint32_t* __restrict__ flag,
                               uint32_t* __restrict__ hist, int64_t item) {
  __shared__ uint32_t h[kBins];
  const Item it = items[item];
  if (flag && !flag[it.tensor]) return;  // block-uniform
  for (int b = threadIdx.x; b < kBins; b += kThreads) h[b] = 0;
  __syncthreads();
  for (int64_t b = it.begin; b < it.end; b += kSub) {
    const int64_t end = min(b + kSub, it.end);
#pragma unroll 4
    for (int k = 0; k < kV; ++k) {
      const int64_t e = b + 4 * ((int64_t)k * kThreads + threadIdx.x);
      if (e >= end) continue;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      const bool full = e + 4 <= end;
      const int nv = full ? 4 : (int)(end - e);
      if (full) {
        const float4 xv = *reinterpret_cast<const float4*>(x + e);
        float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE == 1) rv = *reinterpret_cast<const float4*>(r + e);
        v[0] = tprime<MODE>(xv.x, rv.x, alpha);
        v[1] = tprime<MODE>(xv.y, rv.y, alpha);
        v[2] = tprime<MODE>(xv.z, rv.z, alpha);
        v[3] = tprime<MODE>(xv.w, rv.w, alpha);
        if (MODE != 0) *reinterpret_cast<float4*>(r + e) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        for (int c = 0; c < nv; ++c) {
          v[c] = tprime<MODE>(x[e + c], MODE == 1 ? r[e + c] : 0.0f, alpha);
          if (MODE != 0) r[e + c] = v[c];
        }
      }
      for (int c = 0; c < nv; ++c) atomicAdd(&h[mag_key(v[c]) >> kShift], 1u);
    }
  }
  __syncthreads();
  uint32_t* ht = hist + (size_t)it.tensor * kBins;
  for (int b = threadIdx.x; b < kBins; b += kThreads)
    if (h[b]) atomicAdd(&ht[b], h[b]);
}
template <int MODE>
__global__ __launch_bounds__(kThreads) void topk_prep_hist(
    const float* __restrict__ x, float* __restrict__ r, float alpha, const Item* __restrict__ items,
    uint32_t* __restrict__ hist) {
  prep_hist_item<MODE>(x, r, alpha, items, nullptr, hist, blockIdx.x);
}

// One block per tensor: b1 = max bin with suffix count >= k (flag: only flagged tensors).
__device__ void select_bin_tensor(const uint32_t* __restrict__ hist, const int64_t* __restrict__ kk,
                                  const uint32_t* __restrict__ flag, uint32_t* __restrict__ bin, int t) {
  __shared__ uint32_t s_part[kThreads];
  if (flag && !flag[t]) return;
  const uint32_t* ht = hist + (size_t)t * kBins;
  // thread i owns bins [4i, 4i+4); suffix sums over threads from the top.
  uint32_t c[4], loc = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { c[j] = ht[4 * threadIdx.x + j]; loc += c[j]; }
  s_part[threadIdx.x] = loc;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {  // inclusive suffix scan (Hillis-Steele)
    const uint32_t add = (threadIdx.x + o < kThreads) ? s_part[threadIdx.x + o] : 0u;
    __syncthreads();
    s_part[threadIdx.x] += add;
    __syncthreads();
  }
  const uint64_t k = (uint64_t)kk[t];
  uint64_t above = (threadIdx.x + 1 < kThreads) ? s_part[threadIdx.x + 1] : 0u;  // count in bins > 4i+3
  for (int j = 3; j >= 0; --j) {
    if (above < k && above + c[j] >= k) bin[t] = 4 * threadIdx.x + j;  // exactly one (thread, j) matches
    above += c[j];
  }
}
__global__ __launch_bounds__(kThreads) void topk_select_bin(const uint32_t* __restrict__ hist,
                                                            const int64_t* __restrict__ kk, uint32_t* __restrict__ bin) {
  select_bin_tensor(hist, kk, nullptr, bin, blockIdx.x);
}

// Segment bounds of the exact path's per-tensor sort.
__global__ void topk_segments(int32_t nt, const int64_t* __restrict__ tbegin, const uint32_t* __restrict__ cnt,
                              uint32_t* __restrict__ seg_b, uint32_t* __restrict__ seg_e) {
  for (int32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
    seg_b[t] = (uint32_t)tbegin[t];
    seg_e[t] = (uint32_t)(tbegin[t] + cnt[t]);
  }
}

// Exact-path candidates of one item: every t' (= scale * tp) whose bin is >= b1.
// GLOBAL: composite keys into the item's own region, counted per item (redo: flagged
// tensors only).  Otherwise (|t'|bits << 32 | ~index) appended to the tensor's region
// through one atomic per block pass.
template <bool GLOBAL>
__device__ void collect_item(
    const float* __restrict__ tp, float scale, const Item* __restrict__ items, const int64_t* __restrict__ tbegin,
    const uint32_t* __restrict__ bin, const uint32_t* __restrict__ flag, uint32_t* __restrict__ cnt,
    uint32_t* __restrict__ sub_cnt, uint32_t* __restrict__ item_cnt, uint64_t* __restrict__ cand, int64_t item) {
  __shared__ uint32_t s_wsum[4 * kWaves];
  __shared__ uint32_t s_base;
  const Item it = items[item];
  if (flag && !flag[it.tensor]) return;  // block-uniform
  const uint32_t b1 = bin[it.tensor];
  const int64_t base = tbegin[it.tensor];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int CV = 8;
  constexpr int64_t CS = (int64_t)CV * kThreads * 4;
  const PassCollector col{s_wsum};
  uint32_t item_total = 0;
  for (int64_t b = it.begin; b < it.end; b += CS) {
    const uint32_t lim = (uint32_t)(min(b + CS, it.end) - b);
    const uint32_t off0 = 4u * threadIdx.x;
    float4 v[CV];
    uint32_t selm = 0;
#pragma unroll
    for (int k = 0; k < CV; ++k) {
      const uint32_t o = off0 + 1024u * k;
      float vv[4] = {0.f, 0.f, 0.f, 0.f};
      if (o + 4 <= lim) {
        const float4 t4 = *reinterpret_cast<const float4*>(tp + b + o);
        vv[0] = t4.x; vv[1] = t4.y; vv[2] = t4.z; vv[3] = t4.w;
      } else {
        for (uint32_t c = 0; c < 4 && o + c < lim; ++c) vv[c] = tp[b + o + c];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) vv[c] = __fmul_rn(vv[c], scale);
      v[k] = make_float4(vv[0], vv[1], vv[2], vv[3]);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (o + c < lim && (mag_key(vv[c]) >> kShift) >= b1) selm |= 1u << (4 * k + c);
    }
    if (GLOBAL) {
      item_total += col.append(v, selm, cand + it.begin + item_total, (uint32_t)(b - base) + off0);
      continue;
    }
    const uint32_t nsel = (uint32_t)__popc(selm);
    uint32_t wtot = nsel;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wtot += __shfl_xor(wtot, o, 64);
    if (lane == 0) s_wsum[wave] = wtot;
    __syncthreads();
    uint32_t wpre = 0, tot = 0;
#pragma unroll
    for (int w2 = 0; w2 < kWaves; ++w2) {
      if (w2 < wave) wpre += s_wsum[w2];
      tot += s_wsum[w2];
    }
    if (threadIdx.x == 0) s_base = tot ? atomicAdd(&cnt[it.tensor], tot) : 0u;
    __syncthreads();
    uint64_t* dst = cand + base + s_base + wpre;
    const uint32_t idx0 = (uint32_t)(b - base) + off0;
    const uint64_t lt = (1ull << lane) - 1ull;
    if (wtot) {
#pragma unroll
      for (int k = 0; k < CV; ++k) {
        const float vv[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool sel = (selm >> (4 * k + c)) & 1u;
          const uint64_t m = __ballot(sel);
          if (sel) {
            const uint32_t idx = idx0 + 1024u * k + c;
            dst[__popcll(m & lt)] = ((uint64_t)mag_key(vv[c]) << 32) | (uint64_t)(~idx);
          }
          dst += __popcll(m);
        }
      }
    }
    __syncthreads();  // s_wsum / s_base reuse
  }
  if (GLOBAL && threadIdx.x < kSubsPerItem)  // the item's candidates as one run (sub 0)
    sub_cnt[(size_t)item * kSubsPerItem + threadIdx.x] = threadIdx.x == 0 ? item_total : 0u;
  if (GLOBAL && threadIdx.x == 0) item_cnt[item] = item_total;
}
__global__ __launch_bounds__(kThreads) void topk_collect(
    const float* __restrict__ tp, float scale, const Item* __restrict__ items, const int64_t* __restrict__ tbegin,
    const uint32_t* __restrict__ bin, uint32_t* __restrict__ cnt, uint64_t* __restrict__ cand) {
  collect_item<false>(tp, scale, items, tbegin, bin, nullptr, cnt, nullptr, nullptr, cand, blockIdx.x);
}

// Exact tail: pack every item's candidates at its scanned offset, in order, as device-wide
// sort keys index << 39 | tensor << 31 | (2^31 - 1 - |t'|bits) (a stable sort of the low 39
// bits gives tensor ascending, |t'| descending, index ascending).
__device__ void compact_item(const uint64_t* __restrict__ cand, const Item* __restrict__ items,
                             const uint32_t* __restrict__ sub_cnt, const uint32_t* __restrict__ item_off,
                             uint64_t* __restrict__ packed, int64_t item) {
  __shared__ uint32_t s_pre[kSubsPerItem + 1];
  const Item it = items[item];
  item_prefix(sub_cnt, item, s_pre);
  const uint32_t n = s_pre[kSubsPerItem];
  uint64_t* dst = packed + item_off[item];
  const uint64_t tag = (uint64_t)it.tensor << 31;
  for (uint32_t e = threadIdx.x; e < n; e += kThreads) {
    const uint64_t key = item_key(cand, it.begin, s_pre, e);
    dst[e] = ((key >> 32) << 39) | tag | (uint64_t)(0x7fffffffu - ((uint32_t)key & 0x7fffffffu));
  }
}

// Exact tail, first step: the item's candidate count (item_cnt) and, in the EF modes, the
// residual of every candidate back to t' (the fused pass stored t' - t' there), so the exact
// sort sees the plain t' state.
__device__ void restore_item(const uint64_t* __restrict__ cand, const Item* __restrict__ items,
                             const uint32_t* __restrict__ sub_cnt, const int64_t* __restrict__ tbegin,
                             float* __restrict__ r, uint32_t* __restrict__ item_cnt, int64_t item) {
  __shared__ uint32_t s_pre[kSubsPerItem + 1];
  const Item it = items[item];
  item_prefix(sub_cnt, item, s_pre);
  const uint32_t n = s_pre[kSubsPerItem];
  if (threadIdx.x == 0) item_cnt[item] = n;
  if (!r) return;
  const int64_t base = tbegin[it.tensor];
  for (uint32_t e = threadIdx.x; e < n; e += kThreads) {
    const uint64_t key = item_key(cand, it.begin, s_pre, e);
    r[base + (key >> 32)] = __uint_as_float((uint32_t)key);
  }
}

// Fast path, zero mode (topk_plan_tensor): a tensor with c < k non-zero t' selects all of them
// (ranks [0, c), written by the bucket sort) and then its k - c lowest-index exact zeros, at
// ranks [c, k) in index order — the (|t'| descending, index ascending) order.  Since the tensor
// has only c non-zeros, its first k elements hold at least k - c zeros, so only the 1 Ki-element
// chunks below index k are visited (zmap = (tensor, chunk) pairs of the plan-owned table).  A
// workgroup (kThreads, 4 elements per thread) counts the non-zeros before its chunk (the fused
// pass's per-sub-chunk candidate counts: in zero mode exactly the non-zeros), marks the chunk's
// non-zeros from the candidate keys of its two sub-chunks in an LDS bitmap, and ranks its zeros
// with a block scan; value = t' (the sign of the zero), residual := t' - t' (+0).  Run by the exact
// tail's workgroups when the verdict reports a zero fill and no fallback (round 6; rounds 4-5 ran
// it as a launch of its own, queued by the host after it had read the verdict).
static_assert(kZChunk == 4 * kThreads, "one float4 of a zero-fill chunk per thread");
__device__ void zero_fill_chunk(
    uint2 zm, const uint32_t* __restrict__ zcnt, const int64_t* __restrict__ kk, const int64_t* __restrict__ koff,
    const int64_t* __restrict__ tbegin, const int64_t* __restrict__ tsize, const uint32_t* __restrict__ tfirst,
    const Item* __restrict__ items, const uint32_t* __restrict__ sub_cnt, const uint64_t* __restrict__ cand,
    const float* __restrict__ tp, float scale, float* __restrict__ r, float* __restrict__ values,
    int64_t* __restrict__ indices) {
  __shared__ uint32_t s_bm[kZChunk / 32];
  __shared__ uint32_t s_w[kWaves];
  __shared__ uint32_t s_sum[kWaves];
  const int t = (int)zm.x;
  const uint32_t x = zm.y;  // chunk: sub-chunks 2x and 2x + 1 of the tensor
  const uint32_t c = zcnt[t];
  if (c == kNoZeroFill) return;  // block-uniform
  const int64_t k = kk[t], n = tsize[t], base = tbegin[t];
  const int64_t rel0 = (int64_t)x * kZChunk;
  const uint32_t s0 = tfirst[t] * (uint32_t)kSubsPerItem;
  // non-zeros before this chunk
  uint32_t nz = 0;
  for (uint32_t j = threadIdx.x; j < 2 * x; j += kThreads) nz += sub_cnt[s0 + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_sum[wave] = nz;
  if (threadIdx.x < kZChunk / 32) s_bm[threadIdx.x] = 0;
  __syncthreads();
  uint32_t nzb = 0;
#pragma unroll
  for (int w2 = 0; w2 < kWaves; ++w2) nzb += s_sum[w2];
  const int64_t z = k - (int64_t)c;         // zeros to select
  const int64_t zr0 = rel0 - (int64_t)nzb;  // zeros before this chunk
  if (zr0 >= z) return;                     // block-uniform
#pragma unroll
  for (int h = 0; h < 2; ++h) {  // (every item has kSubsPerItem sub-chunk counts, 0 past the tensor)
    const uint32_t g = s0 + 2 * x + (uint32_t)h;
    const int64_t b = items[g / kSubsPerItem].begin + (int64_t)(g % kSubsPerItem) * kSubPer;
    const uint32_t cx = sub_cnt[g];
    for (uint32_t e = threadIdx.x; e < cx; e += kThreads) {
      const uint32_t rel = (uint32_t)(cand[b + e] >> 32) - (uint32_t)rel0;  // < kZChunk
      atomicOr(&s_bm[rel >> 5], 1u << (rel & 31));
    }
  }
  __syncthreads();
  const uint32_t o = 4u * threadIdx.x;
  const uint32_t bits = (s_bm[o >> 5] >> (o & 31)) & 0xFu;
  uint32_t zmask = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (rel0 + o + q < n && !((bits >> q) & 1u)) zmask |= 1u << q;
  const uint32_t mine = (uint32_t)__popc(zmask);
  uint32_t tot;
  uint32_t pos = block_scan_incl<kThreads>(mine, s_w, tot) - mine;
  const int64_t out0 = koff[t] + (int64_t)c;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (!((zmask >> q) & 1u)) continue;
    const int64_t zr = zr0 + (int64_t)pos++;
    if (zr >= z) break;
    const int64_t idx = rel0 + o + q;
    const float v = __fmul_rn(tp[base + idx], scale);  // +-0
    values[out0 + zr] = v;
    indices[out0 + zr] = idx;
    if (r) r[base + idx] = __fsub_rn(v, v);
  }
}

// The exact path's gather: each tensor's first k sorted keys (|t'|bits << 32 | ~index).
__global__ __launch_bounds__(kThreads) void topk_gather(
    const float* __restrict__ tp, float scale, float* __restrict__ r, const uint64_t* __restrict__ sorted,
    const int64_t* __restrict__ tbegin, const int64_t* __restrict__ tsize, const int64_t* __restrict__ kk,
    const int64_t* __restrict__ koff, float* __restrict__ values, int64_t* __restrict__ indices) {
  const int t = blockIdx.y;
  const int64_t k = kk[t], base = tbegin[t], o = koff[t], n = tsize[t];
  for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < k; j += (int64_t)gridDim.x * kThreads) {
    const uint64_t key = sorted[base + j];
    const uint32_t idx = ~(uint32_t)key;
    if (idx >= n) {  // never expected
      values[o + j] = 0.0f;
      indices[o + j] = -1;
      continue;
    }
    const float v = __fmul_rn(tp[base + idx], scale);
    values[o + j] = v;
    indices[o + j] = (int64_t)idx;
    if (r) r[base + idx] = __fsub_rn(v, v);
  }
}

// ---- the exact tail (round 6): the sampled path's fallback, decided and run on the device
//
// Always enqueued after the bucket kernels, so omf_topk_encode never waits for the plan's verdict
// on the host: a grid of one workgroup per CU (co-resident) reads the verdict words and, unless
// they report a fallback (a redo: a sampled threshold too high for some tensor; an over-full fine
// bin) or the call forces one, runs the zero fill if the verdict reports one and leaves.  On a fallback it runs the exact
// path in phases separated by grid barriers (agent-scope arrivals on a monotone counter, bounded:
// an expiry aborts every workgroup and sets the plan's error word, which omf_plan_check reports
// as OMF_ETIMEOUT):
//   restore    every candidate's residual back to t' (EF modes), per-item candidate counts
//   scan       per-item offsets, per-tensor candidate starts / counts, redo flags (one block)
//   redo       (flagged tensors) a 1024-bin histogram of |t'|, the k-th bin, a re-collection,
//              and the scan again
//   compact    the candidates as keys index << 39 | tensor << 31 | (2^31 - 1 - |t'|bits)
//   sort       an LSD radix sort of the low 39 bits (5 stable passes of 8 bits: per-block digit
//              counts, one block's scan of the digit-major count table, a stable scatter whose
//              in-tile ranks come from wave ballots) — tensor ascending, |t'| descending, index
//              ascending, the order the bucket sort gives
//   gather     values / int64 indices of each tensor's first k keys, residual t' - t' there.
// Sizes come from the device (the candidate count), so nothing is read back to the host.
constexpr int kRadixPasses = (kSortBits + 7) / 8;  // 5
constexpr uint32_t kTailWaitTicks = 20000000u;      // 200 ms of the 100 MHz wall clock: a guard only

struct TailArgs {
  const float* tp;      // t' (EF modes: the residual) or x (mode 0, times scale)
  float scale;
  float* rz;            // the residual (EF modes) or null
  const Item* items;
  int64_t n_items;
  int32_t nt;
  int32_t forced;
  int32_t skip_arrival;  // test hook (omf_plan_set_topk force_fallback 2): the last workgroup skips barrier 1
  const int64_t *kk, *koff, *tbegin;
  const uint32_t *tfirst, *tlast;
  uint32_t *sub_cnt, *item_cnt, *item_off, *cnt, *flag, *hist, *bin;
  int64_t* cstart;
  uint64_t *cand, *packed;  // the candidates' runs; the packed keys (the sort ping-pongs between them)
  uint32_t* gh;             // kRadixDigits x gridDim.x digit counts
  uint32_t* status;         // [0..2] the plan's verdict; [4] arrivals, [5] exits, [6] abort, [7..8] the scan's
  float* values;
  int64_t* indices;
  unsigned long long* stats;  // plan-owned: [0] fast path, [1] zero fills, [2] fallbacks, [3] redos
  uint32_t* err;              // the plan's error word (bit 8: a tail barrier expired)
  const uint2* zmap;          // the zero fill's (tensor, 1 Ki-element chunk) pairs
  uint32_t nzc;
  const uint32_t* zcnt;
  const int64_t* tsize;
};

// Grid barrier of the tail: every workgroup's stores released at agent scope, one arrival on the
// monotone counter status[4], a bounded poll for epoch * gridDim.x arrivals, then an acquire.
// false: aborted (an expiry here or in another workgroup).
__device__ bool tail_sync(const TailArgs& a, uint32_t& epoch) {
  __shared__ uint32_t s_ok;
  __syncthreads();
  ++epoch;
  if (threadIdx.x == 0) {
    __threadfence();
    if (!(a.skip_arrival && epoch == 1 && blockIdx.x == gridDim.x - 1))
      __hip_atomic_fetch_add(&a.status[4], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t target = epoch * gridDim.x;
    const uint64_t t0 = wall_clock64();
    uint32_t ok = 1, polls = 0;
    while (__hip_atomic_load(&a.status[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (__hip_atomic_load(&a.status[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(8);
      if (++polls > 4096u && wall_clock64() - t0 > kTailWaitTicks) {  // never expected
        __hip_atomic_store(&a.status[6], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or(a.err, 8u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    __threadfence();
    s_ok = ok;
  }
  __syncthreads();
  return s_ok != 0u;
}

__device__ __forceinline__ uint32_t ld_word(const uint32_t* p) {
  return __hip_atomic_load(const_cast<uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One LSD pass over keys [0, n) of src (block b owns the tile-aligned range [b, b + 1) * chunk):
// stable by digit (key >> sh) & 255 into dst.  Returns false when a barrier aborted.
__device__ bool tail_radix_pass(const TailArgs& a, uint32_t& epoch, const uint64_t* __restrict__ src,
                                uint64_t* __restrict__ dst, uint32_t n, int sh) {
  __shared__ uint32_t s_h[kRadixDigits];
  __shared__ uint32_t s_wc[kWaves * kRadixDigits];
  __shared__ uint32_t s_part[kWaves];
  const uint32_t G = gridDim.x, b = blockIdx.x, tid = threadIdx.x;
  const uint32_t dmask = (1u << min(8, kSortBits - sh)) - 1u;  // the last pass: bits 32-38 (bit 39 is the index's)
  const uint64_t chunk = (((uint64_t)n + G - 1) / G + kThreads - 1) / kThreads * kThreads;
  const uint32_t b0 = (uint32_t)min((uint64_t)n, b * chunk), b1 = (uint32_t)min((uint64_t)n, b0 + chunk);
  s_h[tid] = 0;  // kThreads == kRadixDigits
  __syncthreads();
  for (uint32_t e = b0 + tid; e < b1; e += kThreads) atomicAdd(&s_h[(uint32_t)(src[e] >> sh) & dmask], 1u);
  __syncthreads();
  a.gh[(size_t)tid * G + b] = s_h[tid];
  if (!tail_sync(a, epoch)) return false;
  if (b == 0) {  // exclusive scan of the digit-major table: thread d owns digit d's G counts
    uint32_t* row = a.gh + (size_t)tid * G;
    uint32_t sum = 0;
    for (uint32_t q = 0; q < G; ++q) sum += row[q];
    uint32_t tot;
    uint32_t run = block_scan_incl<kThreads>(sum, s_part, tot) - sum;
    for (uint32_t q = 0; q < G; ++q) {
      const uint32_t c = row[q];
      row[q] = run;
      run += c;
    }
  }
  if (!tail_sync(a, epoch)) return false;
  __shared__ uint32_t s_run[kRadixDigits];
  s_run[tid] = a.gh[(size_t)tid * G + b];
  const int lane = tid & 63, wave = tid >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  for (uint32_t t0 = b0; t0 < b1; t0 += kThreads) {
    const uint32_t e = t0 + tid;
    const bool valid = e < b1;
    const uint64_t key = valid ? src[e] : 0ull;
    const uint32_t d = (uint32_t)(key >> sh) & dmask;
    uint64_t m = __ballot(valid);  // the lanes of this wave with my digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const uint64_t mb = __ballot(one);
      m &= one ? mb : ~mb;
    }
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s_wc[w * kRadixDigits + tid] = 0;
    __syncthreads();  // (also: s_run complete)
    const uint32_t rank = (uint32_t)__popcll(m & lt);
    if (valid && rank == 0) s_wc[wave * kRadixDigits + d] = (uint32_t)__popcll(m);
    __syncthreads();
    if (valid) {
      uint32_t pos = s_run[d] + rank;
      for (int w = 0; w < wave; ++w) pos += s_wc[w * kRadixDigits + d];
      dst[pos] = key;
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) add += s_wc[w * kRadixDigits + tid];
    s_run[tid] += add;  // (read by other threads only after the next tile's first barrier)
  }
  return tail_sync(a, epoch);
}

__global__ __launch_bounds__(kThreads) void topk_exact_tail(TailArgs a) {
  static_assert(kThreads == kRadixDigits, "one thread per radix digit");
  const uint32_t* st = a.status;
  const uint32_t zf = ld_word(&st[0]), redo = ld_word(&st[1]), over = ld_word(&st[2]);
  const bool fb = a.forced || redo || over;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the plan's counters (omf_topk_stats)
    if (fb) {
      atomicAdd(&a.stats[2], 1ull);
      if (redo) atomicAdd(&a.stats[3], 1ull);
    } else {
      atomicAdd(&a.stats[0], 1ull);
      if (zf) atomicAdd(&a.stats[1], 1ull);
    }
  }
  if (!fb) {  // the usual case: the bucket kernels wrote the selection
    if (zf)     // zero mode: complete the short tensors with their lowest-index zeros
      for (uint32_t c = blockIdx.x; c < a.nzc; c += gridDim.x) {
        __syncthreads();  // (the previous chunk's LDS reads are done)
        zero_fill_chunk(a.zmap[c], a.zcnt, a.kk, a.koff, a.tbegin, a.tsize, a.tfirst, a.items, a.sub_cnt, a.cand,
                        a.tp, a.scale, a.rz, a.values, a.indices);
      }
    return;
  }
  const uint32_t G = gridDim.x;
  uint32_t epoch = 0;
  bool ok = true;
  // restore + item counts
  for (int64_t i = blockIdx.x; i < a.n_items; i += G) {
    __syncthreads();
    restore_item(a.cand, a.items, a.sub_cnt, a.tbegin, a.rz, a.item_cnt, i);
  }
  ok = tail_sync(a, epoch);
  if (ok && blockIdx.x == 0)
    scan_check_block(a.nt, a.kk, a.tfirst, a.tlast, a.item_cnt, a.item_off, a.n_items, a.cstart, a.cnt, a.flag,
                     &a.status[7]);
  ok = ok && tail_sync(a, epoch);
  if (ok && ld_word(&st[8])) {  // a sample set the threshold too high for some tensor: redo it exactly
    for (int64_t i = blockIdx.x; i < a.n_items; i += G) {
      __syncthreads();
      prep_hist_item<0>(a.tp, nullptr, a.scale, a.items, a.flag, a.hist, i);
    }
    ok = tail_sync(a, epoch);
    for (int t = blockIdx.x; ok && t < a.nt; t += G) {
      __syncthreads();
      select_bin_tensor(a.hist, a.kk, a.flag, a.bin, t);
    }
    ok = ok && tail_sync(a, epoch);
    for (int64_t i = blockIdx.x; ok && i < a.n_items; i += G) {
      __syncthreads();
      collect_item<true>(a.tp, a.scale, a.items, a.tbegin, a.bin, a.flag, a.cnt, a.sub_cnt, a.item_cnt, a.cand, i);
    }
    ok = ok && tail_sync(a, epoch);
    if (ok && blockIdx.x == 0)
      scan_check_block(a.nt, a.kk, a.tfirst, a.tlast, a.item_cnt, a.item_off, a.n_items, a.cstart, a.cnt, a.flag,
                       &a.status[7]);
    ok = ok && tail_sync(a, epoch);
  }
  for (int64_t i = blockIdx.x; ok && i < a.n_items; i += G) {
    __syncthreads();
    compact_item(a.cand, a.items, a.sub_cnt, a.item_off, a.packed, i);
  }
  ok = ok && tail_sync(a, epoch);
  const uint32_t n = ok ? ld_word(&st[7]) : 0u;
  uint64_t* src = a.packed;
  uint64_t* dst = a.cand;
  for (int p = 0; ok && p < kRadixPasses; ++p) {
    ok = tail_radix_pass(a, epoch, src, dst, n, 8 * p);
    uint64_t* tmp = src;
    src = dst;
    dst = tmp;
  }
  if (ok) {  // gather: output j of tensor t is the t's sorted key cstart[t] + (j - koff[t])
    const int64_t K = a.koff[a.nt];
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < K; j += (int64_t)G * kThreads) {
      const int t = koff_tensor(a.koff, 0, a.nt - 1, j);
      const uint64_t key = src[a.cstart[t] + (j - a.koff[t])];
      const uint32_t idx = (uint32_t)(key >> 39);
      const int64_t base = a.tbegin[t];
      if ((int)((key >> 31) & 0xFFu) != t) {  // never expected: a key of another tensor
        a.values[j] = 0.0f;
        a.indices[j] = -1;
        continue;
      }
      const float v = __fmul_rn(a.tp[base + idx], a.scale);
      a.values[j] = v;
      a.indices[j] = (int64_t)idx;
      if (a.rz) a.rz[base + idx] = __fsub_rn(v, v);
    }
  }
  // exit: the last workgroup out resets the barrier words for the next call
  __syncthreads();
  if (threadIdx.x == 0 &&
      __hip_atomic_fetch_add(&a.status[5], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1) {
    __hip_atomic_store(&a.status[4], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.status[6], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.status[5], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- host side: the launches
// Workgroups of the exact tail: one per CU (all co-resident, which its grid barriers need), per
// device.
uint32_t tail_grid(int dev) {
  static std::mutex mu;
  static int cus[64] = {0};
  std::lock_guard<std::mutex> lk(mu);
  if (dev < 0 || dev >= 64) return 64u;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 64;
    cus[dev] = std::min(n, 1024);
  }
  return (uint32_t)cus[dev];
}

}  // namespace

size_t omf::topk_sort_tmp_bytes(const omf_plan* p, bool sampled) {  // omf_topk_enc.h
  if (sampled) return 4 * (size_t)kRadixDigits * tail_grid(p->device);  // the exact tail's digit table
  size_t bytes = 0;
  uint64_t* dummy = nullptr;
  uint32_t* off = nullptr;
  (void)rocprim::segmented_radix_sort_keys_desc(nullptr, bytes, dummy, dummy, (unsigned int)p->arena_end,
                                                (unsigned int)p->nt, off, off, 0, 64, (hipStream_t)0, false);
  return bytes;
}

// The zero fill and the fallback (a redo, a fine bin over what a bucket holds, or forced), decided and
// run on the device: leaves at once on a plain fast-path verdict.
int omf::topk_launch_tail(const TopkCall& c, unsigned long long* dstats) {  // omf_topk_enc.h
  const omf_plan* plan = c.plan;
  const TopkKnobs& kn = plan->topk_knobs;
  const EncodeWs& w = c.w;
  const SetupTable& tb = c.tb;
  const TailArgs ta{.tp = c.tp, .scale = c.scale, .rz = c.rz, .items = plan->d_flat, .n_items = plan->n_flat,
                    .nt = plan->nt, .forced = kn.force_fallback != 0 ? 1 : 0,
                    .skip_arrival = kn.force_fallback == 2 ? 1 : 0, .kk = tb.kk, .koff = tb.koff,
                    .tbegin = plan->d_begins, .tfirst = tb.tfirst, .tlast = tb.tlast, .sub_cnt = w.sub_cnt,
                    .item_cnt = w.item_cnt, .item_off = w.item_off, .cnt = w.cnt, .flag = w.flag, .hist = w.hist,
                    .bin = w.bin, .cstart = w.cstart, .cand = w.cand, .packed = w.sorted,
                    .gh = reinterpret_cast<uint32_t*>(w.tmp), .status = w.status, .values = c.values,
                    .indices = c.indices, .stats = dstats, .err = plan->err_word(), .zmap = (const uint2*)tb.zmap,
                    .nzc = (uint32_t)c.host->nzb, .zcnt = w.zcnt, .tsize = plan->d_sizes};
  hipLaunchKernelGGL(topk_exact_tail, dim3(tail_grid(plan->device)), dim3(kThreads), 0, c.st, ta);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf::topk_launch_exact(const TopkCall& c, int64_t kmax, size_t tmp_bytes) {  // omf_topk_enc.h
  const omf_plan* plan = c.plan;
  const EncodeWs& w = c.w;
  const SetupTable& tb = c.tb;
  const int32_t nt = plan->nt;
  const Item* items = plan->d_flat;
  const int64_t* d_begins = plan->d_begins;
  hipStream_t st = c.st;
  const dim3 grid((unsigned)plan->n_flat), blk(kThreads);
  hipLaunchKernelGGL(c.mode == 0 ? topk_prep_hist<0> : c.mode == 1 ? topk_prep_hist<1> : topk_prep_hist<2>, grid, blk, 0,
                     st, c.x, c.residual, c.alpha, items, w.hist);
  hipLaunchKernelGGL(topk_select_bin, dim3((unsigned)nt), blk, 0, st, w.hist, tb.kk, w.bin);
  hipLaunchKernelGGL(topk_collect, grid, blk, 0, st, c.tp, c.scale, items, d_begins, w.bin, w.cnt, w.cand);
  hipLaunchKernelGGL(topk_segments, dim3(((unsigned)nt + kThreads - 1) / kThreads), blk, 0, st, nt, d_begins, w.cnt,
                     w.seg_b, w.seg_e);
  OMF_HIP(hipGetLastError());
  OMF_HIP(rocprim::segmented_radix_sort_keys_desc(w.tmp, tmp_bytes, w.cand, w.sorted, (unsigned int)plan->arena_end,
                                                  (unsigned int)nt, w.seg_b, w.seg_e, 0, 64, st, false));
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((kmax + kThreads - 1) / kThreads, 1024));
  hipLaunchKernelGGL(topk_gather, dim3(gx, (unsigned)nt), blk, 0, st, c.tp, c.scale, c.rz, w.sorted, d_begins,
                     plan->d_sizes, tb.kk, tb.koff, c.values, c.indices);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}
