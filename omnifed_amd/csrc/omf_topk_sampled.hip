// omf_topk_sampled.hip — the Top-K encoder's sampled fast path, MI355X (gfx950): its kernels, every -D tuning override,
// and the launches of a call's pipeline groups (topk_launch_sampled).  Semantics and the host side: omf_topk.hip.
// Kernel map (all tensors of a plan per launch; <= 256 tensors of <= 2^25 elements):
//   1. topk_sample      a hashed sample of t' into a histogram of the top 13 bits of |t'|; per tensor the
//                       threshold bin (below the k-th magnitude with ~6 sigma of margin; tensors too small to
//                       sample keep every element), a "sure" magnitude and the fine-bin map.
//   2. topk_fused       ONE streaming pass: read x (+ residual), write the residual, append every |t'| at or
//                       above the threshold as index << 32 | bits(t') to the 512-element sub-chunk's own range.
//   3. topk_fine_hist   exact fine-bin histogram of the candidates (LDS per super-item).
//   4. topk_scatter_planned (topk_plan + topk_bucket_scatter for large plans): per tensor, the fine bins above
//                       rank k -> buckets of <= 4096 keys with known first ranks, the verdict words (zero fill /
//                       redo / overflow) in the workspace; keys into buckets.
//   5. topk_bucket_sort an LDS sort per bucket -> values / int64 indices ((|t'| desc, index asc)), residual fix-ups.
// Behind them the host side always enqueues topk_exact_tail (omf_topk_exact.hip), which reads the verdict.
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <vector>

#include "omf_topk_enc.h"      // the plan, the layout, the launchers' declarations
#include "omf_topk_enc_dev.h"  // the device steps shared with omf_topk_exact.hip

using namespace omf;
using namespace omf::topk_layout;  // the constants and per-tensor rules shared with the host side
using namespace omf::topk_enc;

namespace {

constexpr int kSShift = 31 - kSBits;
// The threshold bin's margin over the expected k*S/n samples: OMF_THR_Z sigma + OMF_THR_C (a
// performance knob only — a tensor left with fewer than k candidates takes the exact redo).
#ifndef OMF_THR_Z  // -D overrides for a variant library (scripts/exp/variant_lib.sh)
#define OMF_THR_Z 6.0
#endif
#ifndef OMF_THR_C
#define OMF_THR_C 32.0
#endif
constexpr int kFineMaxBits = 18;      // a coarse bin splits by at most the rest of the mantissa
#ifndef OMF_FINE_MARGIN  // a -D override for a variant library (scripts/exp/variant_lib.sh)
#define OMF_FINE_MARGIN 8
#endif
constexpr int kFineMargin = OMF_FINE_MARGIN;  // a fine bin expects <= kBucketHalf / 8 elements
constexpr int kBT = 512;              // bucket-sort block: 512 threads x 8 keys = 2 kBucketHalf
constexpr int kBI = 8;
constexpr int kPlanMaxBuckets = (1 << 25) / kBucketHalf + 2;  // topk_plan's rule (no big-bin buckets)
constexpr int kMaxBigBins = 128;  // kept fine bins over kBucketHalf keys per tensor on the fast path
constexpr int kSubThreads = kSubPer / 4;      // one float4 per thread: 128 threads, two waves
constexpr int kSubWaves = kSubThreads / 64;

__device__ __forceinline__ uint32_t hash32(uint32_t h) {  // murmur3 finaliser
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}

// Passes 1+2 (one launch, topk_sample): R = ceil(n / stride) runs, stride = max(256,
// ceil(n / max_runs)); run j covers 16 aligned elements at j*stride + 16 * (hash(.) % (span/16))
// (a whole 64-byte sector: random sectors, not elements, are what the sample costs), so
// S <= 16 R samples go into a histogram of the top 13 bits of |t'|; then the bin whose
// suffix holds k*S/n + 6 sqrt(k*S/n) + 32 samples (0 = every element, for tensors too small
// to sample).  Four lanes read one run (float4 each).
// Sampling is split over the tensor's runs: kSRunsPerBlock runs per block (a 16 Ki-run tensor
// is 32 blocks on 32 CUs instead of one CU doing all its loads and contended LDS histogram
// atomics), each block adding its LDS histogram's non-empty bins into the tensor's global
// histogram gh.  The LAST block of a tensor to arrive (a per-tensor counter, reset by that
// block) reads and clears gh with atomic RMWs — performed where the other blocks' atomics
// were — and derives the tensor's threshold, "sure" bin and fine-bin map
// (sample_threshold_tensor), so no second launch and no tail of one-block-per-tensor work
// after the last sample.  smap: per block, (tensor, first run).  Block 0 also clears this
// call's status words.
#ifndef OMF_SAMPLE_HIST_LATE  // experiment builds: 0 clears the redo histogram before the threshold's barriers
#define OMF_SAMPLE_HIST_LATE 1
#endif

// The tensor's threshold from its sample histogram h (LDS, kSBins, loaded; 1024 threads) of
// the non-zero samples and its count of exact-zero samples `zeros`: the threshold bin — the bin
// whose suffix holds k*S/n + 6 sqrt(k*S/n) + 32 of the S samples — the "sure" bin, and the
// fine-bin map.  The threshold is stored as a magnitude key (tkey): bin << 18, or 1 — every
// non-zero element, the zeros excluded — when the target is not reached above bin 0 (too few
// samples to trust, or fewer non-zero samples than the target: an exact-zero-heavy tensor such
// as the PS's average of sparse Top-K updates).  Exact zeros are never candidates: when a tensor
// has fewer than k non-zeros, its selection is completed by its lowest-index zeros (topk_plan
// and the zero fill, zero_fill_chunk), the order the exact path's stable sort gives ties.
// Also clears the tensor's redo histogram and its fine bins.
__device__ void sample_threshold_tensor(
    int t, int64_t n, const uint32_t* h, uint32_t zeros, float2 sure_zc, const int64_t* __restrict__ kk,
    const uint32_t* __restrict__ tfirst, const uint32_t* __restrict__ tlast, uint32_t* __restrict__ tkey,
    uint32_t* __restrict__ hist, uint32_t* __restrict__ item_cnt, uint32_t* __restrict__ thi,
    uint32_t* __restrict__ fmap, uint32_t* __restrict__ tlo, uint32_t* __restrict__ fcount,
    uint32_t* __restrict__ fhist) {
  constexpr int PER = kSBins / 1024;
  __shared__ uint32_t s_w[16];
  // (the redo histogram is cleared after the last barrier below: a workgroup barrier waits for the
  // workgroup's outstanding stores, so stores issued here would delay every block scan)
#if !OMF_SAMPLE_HIST_LATE
  for (int b = threadIdx.x; b < kBins; b += 1024) hist[(size_t)t * kBins + b] = 0;
#endif
  uint32_t c[PER], loc = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = h[PER * threadIdx.x + j];
    loc += c[j];
  }
  uint32_t S;
  const uint32_t above0 = [&] {  // samples in the bins of higher threads
    const uint32_t inc = block_scan_incl<1024>(loc, s_w, S);
    return S - inc;
  }();
  S += zeros;  // every sample, for the expected counts
  const double m = (double)kk[t] * (double)S / (double)max(n, (int64_t)1);
  const double want = m + (double)OMF_THR_Z * sqrt(m) + (double)OMF_THR_C;
  __shared__ uint32_t s_thr, s_hikey, s_min, s_max;
  if (threadIdx.x == 0) {
    s_thr = 0;
    s_hikey = 0x80000000u;  // above every magnitude key: nothing sure
    s_min = kSBins;
    s_max = 0;
  }
  __syncthreads();
  if (!(m < 16.0 || want >= (double)S)) {  // else too few samples to trust: keep every element
    const uint32_t target = (uint32_t)ceil(want);
    uint32_t above = above0;
    for (int j = PER - 1; j >= 0; --j) {
      if (above < target && above + c[j] >= target) s_thr = PER * threadIdx.x + j;  // exactly one match
      above += c[j];
    }
    // The "sure" bin: every bin from it up holds, with a margin of sure_zc (1.5 sigma + 2 by
    // default), fewer than k elements in total, so its elements are taken as selected (the fused
    // pass zeroes their residual; the bucket kernels give a sure key past rank k its t' back).
    const double sure = m - (double)sure_zc.x * sqrt(m) - (double)sure_zc.y;
    if (sure >= 1.0) {
      const uint32_t ts = (uint32_t)sure;
      above = above0;
      for (int j = PER - 1; j >= 0; --j) {
        if (above <= ts && above + c[j] > ts) {  // exactly one crossing: bin b holds rank ts
          // the sure magnitude inside bin b, interpolated linearly (magnitude is linear in the
          // key bits within a bin): the top (ts - above) / c of the bin's samples are sure
          const uint32_t b = PER * threadIdx.x + j;
          const double f = (double)(ts - above) / (double)c[j];
          s_hikey = ((b + 1u) << kSShift) - (uint32_t)(f * (double)(1u << kSShift));
        }
        above += c[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (c[j]) {
      atomicMin(&s_min, (uint32_t)(PER * threadIdx.x + j));
      break;
    }
#pragma unroll
  for (int j = PER - 1; j >= 0; --j)
    if (c[j]) {
      atomicMax(&s_max, (uint32_t)(PER * threadIdx.x + j));
      break;
    }
  __syncthreads();
  const uint32_t thr = s_thr;
  // Fine bins of the candidates (the exact per-tensor histogram the bucket sort plans from):
  // coarse bin lo + i (i < 1024) is split into 2^r_i fine bins by the next r_i bits of |t'|,
  // r_i sized from this sample so that a fine bin expects <= kBucketHalf / mg elements,
  // estimating a coarse bin's elements by an upper bound (h + 3 sqrt(h) + 3) n / S of its h
  // samples (a bin the sample missed can still hold ~3 n / S), up to two bins above the
  // largest sampled one.
  const uint32_t lo = thr > 0 ? thr : (s_min < (uint32_t)kSBins ? s_min : 0u);
  const uint32_t cb = lo + threadIdx.x;
  const double scale = (double)n / (double)max(S, 1u);
  double est = 0.0;
  if (cb < (uint32_t)kSBins && cb <= s_max + 2) {
    const double hb = (double)h[cb];
    est = (hb + 3.0 * sqrt(hb) + 3.0) * scale;
  }
  uint32_t rbits = 0, F = 0, inc = 0;
  for (int mg = kFineMargin; mg >= 0; mg >>= 1) {
    rbits = 0;
    if (mg > 0) {
      const double need = est * (double)mg / (double)kBucketHalf;
      while (rbits < kFineMaxBits && (double)(1u << rbits) < need) ++rbits;
    }
    inc = block_scan_incl<1024>(1u << rbits, s_w, F);  // fine-bin counts
    if (F <= (uint32_t)kFineMax || mg == 0) break;
  }
  const uint32_t off = inc - (1u << rbits);
  fmap[(size_t)t * kCoarse + threadIdx.x] = off | (rbits << 16);
  if (threadIdx.x == 0) {
    tkey[t] = thr > 0 ? thr << kSShift : 1u;  // 1: every non-zero (zero mode)
    thi[t] = max(s_hikey, (thr + 1u) << kSShift);  // a magnitude key: sure keys are candidates
    tlo[t] = lo;
    fcount[t] = F;
  }
  for (uint32_t i = threadIdx.x; i < F; i += 1024) fhist[(size_t)t * kFineMax + i] = 0;
#if OMF_SAMPLE_HIST_LATE
  for (int b = threadIdx.x; b < kBins; b += 1024) hist[(size_t)t * kBins + b] = 0;  // this call's redo histogram
#endif
}

template <int MODE>
__global__ __launch_bounds__(1024) void topk_sample(
    const float* __restrict__ x, const float* __restrict__ r, float alpha, const int64_t* __restrict__ tbegin,
    const int64_t* __restrict__ tsize, const uint32_t* __restrict__ smap, int64_t max_runs, uint32_t* __restrict__ gh,
    uint32_t* __restrict__ gz, uint32_t* __restrict__ arrive, uint32_t* __restrict__ status,
    const int64_t* __restrict__ kk, const uint32_t* __restrict__ tfirst, const uint32_t* __restrict__ tlast,
    uint32_t* __restrict__ tkey, uint32_t* __restrict__ hist, uint32_t* __restrict__ item_cnt,
    uint32_t* __restrict__ thi, uint32_t* __restrict__ fmap, uint32_t* __restrict__ tlo, uint32_t* __restrict__ fcount,
    uint32_t* __restrict__ fhist, uint32_t blk0, float2 sure_zc) {
  constexpr int kLanesPerRun = kSRun / 4;  // one float4 per lane
  constexpr int kGroups = 1024 / kLanesPerRun;
  constexpr int U = kSRunsPerBlock / kGroups;  // runs per lane group, all loads in flight at once
  static_assert(U * kGroups == kSRunsPerBlock && U >= 1, "runs per block: a multiple of the lane groups");
  __shared__ uint32_t h[kSBins];
  __shared__ uint32_t s_last, s_zero;
  const uint32_t bid = blk0 + blockIdx.x;  // launches cover ranges of tensors (pipeline groups)
#ifdef OMF_EXP_SAMPLE_TS  // experiment builds: per-phase wall-clock stamps of a few sample blocks
  const uint64_t ts0 = wall_clock64();
#endif
  const int t = (int)smap[2 * bid];
  const int64_t r0 = smap[2 * bid + 1];
  if (bid == 0 && threadIdx.x < 9) status[threadIdx.x] = 0u;  // the verdict and the exact tail's words
  for (int b = threadIdx.x; b < kSBins; b += 1024) h[b] = 0;
  if (threadIdx.x == 0) s_zero = 0;
  const int64_t base = tbegin[t], n = tsize[t];
  const int64_t stride = sample_stride(n, max_runs), nr = sample_runs(n, stride);
  const int64_t r1 = min(r0 + (int64_t)kSRunsPerBlock, nr);
  const uint32_t salt = (uint32_t)t * 0x9E3779B9u;
  const int q = threadIdx.x & (kLanesPerRun - 1);  // float4 of the run
  float4 xv[U], rv[U];
  int64_t rel[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {  // every load issued unconditionally (no branch around a load:
    // hipcc would wait for each one in turn); past-the-end runs clamped
    const int64_t j = min(r0 + (int64_t)(threadIdx.x / kLanesPerRun) + (int64_t)u * kGroups, r1 - 1);
    const int64_t lo = j * stride;
    const int64_t span = min(stride, n - lo);
    const int64_t runs = max((int64_t)1, span / kSRun);
    rel[u] = lo + kSRun * (int64_t)(hash32((uint32_t)lo ^ salt) % (uint32_t)runs) + 4 * q;
    const int64_t e = base + min(rel[u], (n - 1) & ~(int64_t)3);  // 16-byte aligned, inside the arena
    xv[u] = *reinterpret_cast<const float4*>(x + e);
    rv[u] = MODE == 1 ? *reinterpret_cast<const float4*>(r + e) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();  // h cleared
#ifdef OMF_EXP_SAMPLE_TS
  const uint64_t ts1 = wall_clock64();
#endif
  uint32_t zc = 0;  // exact-zero samples: counted apart (one LDS atomic per wave, not per sample)
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (r0 + (int64_t)(threadIdx.x / kLanesPerRun) + (int64_t)u * kGroups >= r1) continue;
    const float xs[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
    const float rs[4] = {rv[u].x, rv[u].y, rv[u].z, rv[u].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (rel[u] + c >= n) continue;
      const uint32_t key = mag_key(tprime<MODE>(xs[c], rs[c], alpha));
      if (key) atomicAdd(&h[key >> kSShift], 1u);
      else ++zc;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) zc += __shfl_xor(zc, o, 64);
  if ((threadIdx.x & 63) == 0 && zc) atomicAdd(&s_zero, zc);
  __syncthreads();
  const uint32_t nblk = sample_blocks(nr);
  if (nblk == 1) {  // the tensor's whole sample is in this block's histogram (the usual case)
#ifdef OMF_EXP_SAMPLE_TS
    const uint64_t ts2 = wall_clock64();
#endif
    sample_threshold_tensor(t, n, h, s_zero, sure_zc, kk, tfirst, tlast, tkey, hist, item_cnt, thi, fmap, tlo, fcount,
                            fhist);
#ifdef OMF_EXP_SAMPLE_TS
    __syncthreads();
    const uint64_t ts3 = wall_clock64();
    if (threadIdx.x == 0 && (t == 0 || t == 1 || t == 2 || t == 50 || t == 100 || t == 181 || t == 182))
      printf("SAMPLE_TS t=%d n=%lld start=%llu load+clear=%llu hist=%llu thr=%llu\n", t, (long long)n,
             (unsigned long long)ts0, (unsigned long long)(ts1 - ts0), (unsigned long long)(ts2 - ts1),
             (unsigned long long)(ts3 - ts2));
#endif
    return;
  }
  uint32_t* g = gh + (size_t)t * kSBins;
  for (int b = threadIdx.x; b < kSBins; b += 1024)
    if (h[b]) atomicAdd(&g[b], h[b]);
  if (threadIdx.x == 0 && s_zero) atomicAdd(&gz[t], s_zero);
  // Arrival (cdna_hip_programming.md §6 Guideline 16, row 1): every wave waits for its
  // histogram atomics (vmcnt(0); agent-scope RMWs are performed past the XCD's L2), a workgroup
  // barrier, then one agent-scope add.  No __threadfence: on gfx950 an agent-scope release
  // writes back the whole L2, and one per wave of ~3 000 blocks cost over a millisecond.
  drain_vmem();
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = add_agent(&arrive[t], 1u) == nblk - 1;
    if (last) __hip_atomic_store(&arrive[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next call
    s_last = last ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  for (int b = threadIdx.x; b < kSBins; b += 1024) h[b] = atomicExch(&g[b], 0u);  // read + clear for the next call
  if (threadIdx.x == 0) s_zero = atomicExch(&gz[t], 0u);
  __syncthreads();
  sample_threshold_tensor(t, n, h, s_zero, sure_zc, kk, tfirst, tlast, tkey, hist, item_cnt, thi, fmap, tlo, fcount,
                          fhist);
}

// Fine bin of a candidate magnitude (monotone in mag; below / above the mapped range clamp
// to the lowest / highest fine bin), and the key's position inside its fine bin: the low `wbits`
// bits of |t'| (0 bits for the clamped bottom / top bins).
// Bit arithmetic only (hipcc turns selects here into branches, and waits for a load issued under
// a branch at the branch's end, which serialised the loads of the unrolled loops that call this):
// out-of-range coarse bins go to fine bin 0 (below) or F - 1 (above) with no low bits.
__device__ __forceinline__ uint32_t fine_map_entry(uint32_t mag, uint32_t lo, const uint32_t* __restrict__ map_t) {
  const int c = (int)(mag >> kSShift) - (int)lo;
  return map_t[min(max(c, 0), kCoarse - 1)];
}

// The fine bin from the coarse bin's map entry m (fine_map_entry).
__device__ __forceinline__ uint32_t fine_bin_from(uint32_t mag, uint32_t lo, uint32_t m, uint32_t F, uint32_t& low,
                                                  uint32_t& wbits) {
  const int c = (int)(mag >> kSShift) - (int)lo;
  const uint32_t r = m >> 16;
  const uint32_t below = (uint32_t)(c >> 31), above = (uint32_t)((kCoarse - 1 - c) >> 31);  // all ones or 0
  wbits = (kSShift - r) & ~(below | above);
  low = mag & ((1u << wbits) - 1u);
  const uint32_t fb = (m & 0xffffu) + ((mag >> (kSShift - r)) & ((1u << r) - 1u));
  return min((fb | above) & ~below, F - 1u);  // an in-range fine bin is < F
}

__device__ __forceinline__ uint32_t fine_bin_pos(uint32_t mag, uint32_t lo, const uint32_t* __restrict__ map_t,
                                                 uint32_t F, uint32_t& low, uint32_t& wbits) {
  return fine_bin_from(mag, lo, fine_map_entry(mag, lo, map_t), F, low, wbits);
}

__device__ __forceinline__ uint32_t fine_bin(uint32_t mag, uint32_t lo, const uint32_t* __restrict__ map_t,
                                             uint32_t F) {
  uint32_t low, wbits;
  return fine_bin_pos(mag, lo, map_t, F, low, wbits);
}

// Pass 3: t' (written to the residual in the EF modes) and the candidates above the
// sampled threshold.  One 128-thread block per 512-element sub-chunk of an item (sub j of
// item i is block 32 i + j), one float4 of x (and r) per thread: the shape that streams
// fastest here (scripts/exp/ef_probe.py: r += x at 5.6 TB/s with one float4 per thread vs
// 5.1 with 8 per thread or a persistent grid; round 5, scripts/exp/dec_shapes.hip: 0.733 ms
// for Llama-400M's 12 N with 128-thread blocks against 0.763 with 256, 0.793 with 512).  The sub's candidates go to its own element
// range of `cand` in index order (one wave scan + one barrier), its count to sub_cnt.
// MODE 0: t' = alpha x (not stored); 1: r := r + alpha x; 2: r := alpha x.
template <int MODE>
__global__ __launch_bounds__(kSubThreads) void topk_fused(
    const float* __restrict__ x, float* __restrict__ r, float alpha, const Item* __restrict__ items,
    const int64_t* __restrict__ tbegin, const uint32_t* __restrict__ tkey, const uint32_t* __restrict__ thi,
    uint32_t* __restrict__ sub_cnt, uint32_t* __restrict__ item_cnt, uint64_t* __restrict__ cand, uint32_t sub0) {
  __shared__ uint32_t s_w[kSubWaves];
  const uint32_t bid = sub0 + blockIdx.x;
  const Item it = items[bid / kSubsPerItem];
  const int64_t b = it.begin + (int64_t)(bid % kSubsPerItem) * kSubPer;
  if (b >= it.end) {  // past a tensor's last sub-chunk
    if (threadIdx.x == 0) sub_cnt[bid] = 0;
    return;
  }
  const uint32_t thr = tkey[it.tensor], hi = thi[it.tensor];
  const int64_t base = tbegin[it.tensor];
  const uint32_t lim = (uint32_t)(min(b + kSubPer, it.end) - b);
  const uint32_t o = 4u * threadIdx.x;
  // EF modes store t' - t' (0, or NaN for an infinite t') for the "sure" elements (|t'| key >= hi:
  // taken as selected, sure_margin()) and t' for the rest; the bucket kernels then zero only
  // the selected keys below the sure bin (and restore a sure key that was not selected).
  float vv[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t selm = 0;
  const bool full = o + 4 <= lim;
  if (full) {
    const f32x4_t xl = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(x + b + o));  // read once
    const float4 xv = make_float4(xl[0], xl[1], xl[2], xl[3]);
    float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MODE == 1) {
      const f32x4_t rl = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(r + b + o));
      rv = make_float4(rl[0], rl[1], rl[2], rl[3]);
    }
    vv[0] = tprime<MODE>(xv.x, rv.x, alpha);
    vv[1] = tprime<MODE>(xv.y, rv.y, alpha);
    vv[2] = tprime<MODE>(xv.z, rv.z, alpha);
    vv[3] = tprime<MODE>(xv.w, rv.w, alpha);
  } else {
    for (uint32_t c = 0; c < 4 && o + c < lim; ++c)
      vv[c] = tprime<MODE>(x[b + o + c], MODE == 1 ? r[b + o + c] : 0.0f, alpha);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (o + c < lim && mag_key(vv[c]) >= thr) selm |= 1u << c;
  if (MODE != 0) {
    float rr[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) rr[c] = mag_key(vv[c]) >= hi ? __fsub_rn(vv[c], vv[c]) : vv[c];
    if (full) store_nt(r + b + o, make_float4(rr[0], rr[1], rr[2], rr[3]));
    else
      for (uint32_t c = 0; c < 4 && o + c < lim; ++c) r[b + o + c] = rr[c];
  }
  // ordered positions: wave inclusive scan of the counts, then the waves before mine
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t mine = (uint32_t)__popc(selm);
  uint32_t inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(inc, d, 64);
    if (lane >= d) inc += u;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint32_t pos = inc - mine, total = 0;
#pragma unroll
  for (int w2 = 0; w2 < kSubWaves; ++w2) {
    const uint32_t ws = s_w[w2];
    if (w2 < wave) pos += ws;
    total += ws;
  }
  if (selm) {
    uint64_t* dst = cand + b;
    const uint32_t idx0 = (uint32_t)(b - base) + o;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if ((selm >> c) & 1u) dst[pos++] = ((uint64_t)(idx0 + c) << 32) | (uint64_t)__float_as_uint(vv[c]);
  }
  if (threadIdx.x == 0) sub_cnt[bid] = total;  // (the fallback sums an item's subs: topk_item_counts)
}

// Fast path: a "super-item" is up to kSupItems consecutive items (16 Ki-element chunks) of one
// tensor, handled by one 1024-thread block so that per-tensor LDS tables (fine-bin counts,
// bucket counts) aggregate many keys before touching global memory.  SupView maps the block
// to its tensor and lists its candidates (sub-chunk runs, in index order).
struct SupView {
  uint32_t* s_spre;   // [1025] exclusive prefix of the runs' counts
  int64_t* s_ibeg;    // [kSupItems] arena offsets of the items
  int t;
  uint32_t total;
  bool first;  // the tensor's first super-item
  // supinfo[sup] = {tensor, first item, items, first} (a plan-owned table: no search), and the
  // tensor's fine-bin map staged into s_map[kCoarse] (read per key by the callers).
  __device__ __forceinline__ void init(const uint4* __restrict__ supinfo, const Item* __restrict__ items,
                                       const uint32_t* __restrict__ sub_cnt, const uint32_t* __restrict__ fmap,
                                       uint32_t* s_map, uint32_t* s_part, uint32_t sup) {
    const uint4 si = supinfo[sup];
    t = (int)si.x;
    first = si.w != 0u;
    const uint32_t i0 = si.y, ni = si.z;
    s_map[threadIdx.x] = fmap[(size_t)t * kCoarse + threadIdx.x];  // 1024 threads = kCoarse
    const uint32_t run = threadIdx.x;  // run j of item j / kSubsPerItem
    const uint32_t c = run < ni * kSubsPerItem ? sub_cnt[(size_t)i0 * kSubsPerItem + run] : 0u;
    if (threadIdx.x < ni) s_ibeg[threadIdx.x] = items[i0 + threadIdx.x].begin;
    uint32_t tot;
    s_spre[threadIdx.x + 1] = block_scan_incl<1024>(c, s_part, tot);
    if (threadIdx.x == 0) s_spre[0] = 0;
    __syncthreads();
    total = s_spre[1024];
  }
  // arena position of candidate e (< total) in the cand buffer
  __device__ __forceinline__ int64_t pos(uint32_t e) const {
    int j = 0;  // the run with s_spre[j] <= e < s_spre[j + 1]
#pragma unroll
    for (int h = 512; h > 0; h >>= 1)
      if (s_spre[j + h] <= e) j += h;
    return s_ibeg[j / kSubsPerItem] + (int64_t)(j % kSubsPerItem) * kSubPer + (e - s_spre[j]);
  }
};

// Fast path, pass H: the exact fine-bin histogram of every tensor's candidates (LDS counts per
// super-item, flushed with one global atomic per touched bin).
#ifndef OMF_FHIST_U  // 4: measured against 8 (30.9 us, more VGPRs) on Llama-400M
#define OMF_FHIST_U 4
#endif
__global__ __launch_bounds__(1024) void topk_fine_hist(
    const uint64_t* __restrict__ cand, const Item* __restrict__ items, const uint32_t* __restrict__ sub_cnt,
    const uint4* __restrict__ supinfo, const uint32_t* __restrict__ fmap, const uint32_t* __restrict__ tlo,
    const uint32_t* __restrict__ fcount, uint32_t* __restrict__ fhist, const uint32_t* __restrict__ bbase,
    uint32_t* __restrict__ bfill, uint32_t sup0) {
  __shared__ uint32_t s_h[kFineMax];
  __shared__ uint32_t s_spre[1025], s_part[1024];
  __shared__ int64_t s_ibeg[kSupItems];
  __shared__ uint32_t s_map[kCoarse];
  SupView v{s_spre, s_ibeg, 0, 0, false};
  for (int i = threadIdx.x; i < kFineMax; i += 1024) s_h[i] = 0;
  v.init(supinfo, items, sub_cnt, fmap, s_map, s_part, sup0 + blockIdx.x);
  const uint32_t lo = tlo[v.t], F = fcount[v.t];
  if (v.first)  // the tensor's bucket reservation counters, for topk_scatter_planned (topk_plan also clears them)
    for (uint32_t j = bbase[v.t] + threadIdx.x; j < bbase[v.t + 1]; j += 1024) bfill[j] = 0;
  const uint32_t* map_t = s_map;
  constexpr int U = OMF_FHIST_U;  // key loads in flight per thread
  for (uint32_t e0 = threadIdx.x; e0 < v.total; e0 += U * 1024) {
    uint64_t key[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t e = min(e0 + (uint32_t)u * 1024, v.total - 1);
      key[u] = cand[v.pos(e)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (e0 + (uint32_t)u * 1024 < v.total)
        atomicAdd(&s_h[fine_bin((uint32_t)key[u] & 0x7fffffffu, lo, map_t, F)], 1u);
  }
  __syncthreads();
  uint32_t* h = fhist + (size_t)v.t * kFineMax;
  for (uint32_t i = threadIdx.x; i < F; i += 1024)
    if (s_h[i]) atomicAdd(&h[i], s_h[i]);
}

// Fast path, plan (one block per tensor): suffix counts of the fine bins from the top; the
// bins that start above rank k are kept, bin i goes to bucket floor(se_i / kBucketHalf)
// (se_i = keys in higher bins), a bucket starts at its smallest se.  A tensor with fewer than
// k candidates is flagged for the exact redo — unless its threshold was every non-zero (zero
// mode, tkey == 1): then every candidate is selected (ranks [0, c)) and the rest of its
// selection is its k - c lowest-index exact zeros, written by zero_fill_chunk; zcnt[t] = c for
// such a tensor, 0xffffffff otherwise.  Flags the call for the fallback sort when a kept fine
// bin holds more than kBucketHalf keys.  status[0] |= zero fill, [1] |= redo, [2] |= overflow.
__device__ void topk_plan_tensor(
    int t, const int64_t* __restrict__ kk, const uint32_t* __restrict__ fcount, const uint32_t* __restrict__ fhist,
    const uint32_t* __restrict__ bbase, int32_t* __restrict__ fbucket, uint32_t* __restrict__ bstart,
    BucketRec* __restrict__ brec, uint32_t* __restrict__ bfill, const int64_t* __restrict__ kb2,
    uint32_t* __restrict__ flag, uint32_t* __restrict__ status, const uint32_t* __restrict__ tkey,
    uint32_t* __restrict__ zcnt, int dbg) {
  constexpr int PER = kFineMax / 1024;
  __shared__ uint32_t s_bs[kPlanMaxBuckets];
  __shared__ uint32_t part[1024];
  __shared__ uint32_t s_kend, s_nb, s_over;
  const uint32_t F = fcount[t];
  const bool zero_mode = tkey[t] == 1u;
  uint64_t k = (uint64_t)kk[t];
  const uint32_t b0 = bbase[t], nbmax = bbase[t + 1] - b0;
  const uint32_t nbl = min(nbmax, (uint32_t)kPlanMaxBuckets);  // this rule's buckets: se / kBucketHalf < nbl
  const uint32_t* ht = fhist + (size_t)t * kFineMax;
  uint32_t h[PER], loc = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const uint32_t i = PER * threadIdx.x + j;
    h[j] = i < F ? ht[i] : 0u;
    loc += h[j];
  }
  if (threadIdx.x == 0) {
    s_kend = 0;
    s_nb = 0;
    s_over = 0;
  }
  for (uint32_t j = threadIdx.x; j < nbl; j += 1024) s_bs[j] = 0xffffffffu;
  uint32_t tot32;
  const uint32_t inc = block_scan_incl<1024>(loc, part, tot32);
  const uint64_t total = tot32;
  if (total < k && !zero_mode) {  // the sampled threshold was too high: exact redo (fallback path)
    if (threadIdx.x == 0) {
      flag[t] = 1u;
      zcnt[t] = kNoZeroFill;
      atomicOr(&status[1], 1u);
    }
    for (uint32_t j = threadIdx.x; j < nbmax; j += 1024) brec[b0 + j] = BucketRec{0, 0, 0};
    return;
  }
  const bool zero_fill = total < k;  // zero mode: every candidate selected, then zeros
  if (threadIdx.x == 0) {
    zcnt[t] = zero_fill ? tot32 : kNoZeroFill;
    if (zero_fill) atomicOr(&status[0], 1u);
  }
  if (zero_fill) k = total;  // the lowest candidate bin ends the kept range
  uint64_t se = tot32 - inc;  // keys in the bins of higher threads
  int32_t* fb = fbucket + (size_t)t * kFineMax;
  for (int j = PER - 1; j >= 0; --j) {
    const uint32_t i = PER * threadIdx.x + j;
    int32_t bucket = -1;
    if (h[j] && se < k) {
      bucket = (int32_t)(se / kBucketHalf);
      atomicMin(&s_bs[bucket], (uint32_t)se);
      if (h[j] > (uint32_t)kBucketHalf) {
        s_over = 1u;
        if (dbg & 8) printf("omf_topk plan: tensor %d fine bin %u of %u holds %u (se %llu k %llu)\n", t, i, F, h[j],
                            (unsigned long long)se, (unsigned long long)k);
      }
      if (se + h[j] >= k) {  // the bin of the k-th key (exactly one)
        s_kend = (uint32_t)(se + h[j]);
        s_nb = (uint32_t)bucket + 1u;
      }
    }
    if (i < F) fb[i] = bucket;
    se += h[j];
  }
  __syncthreads();
  const uint32_t nb = s_nb;
  for (uint32_t j = threadIdx.x; j < nbmax; j += 1024) {
    const uint32_t g = b0 + j;
    uint32_t st = 0, c = 0;
    if (j < nb && j < nbl && s_bs[j] != 0xffffffffu) {
      st = s_bs[j];
      const uint32_t en = j + 1 < nb ? s_bs[j + 1] : s_kend;
      c = en > st ? en - st : 0u;
    }
    bstart[g] = st;
    brec[g] = BucketRec{(uint64_t)kb2[t] + st, st, min(c, 0xffffu) | ((uint32_t)t << 16)};
    bfill[g] = 0;
  }
  if (threadIdx.x == 0) {
    flag[t] = 0;
    if (s_over) atomicOr(&status[2], 1u);
  }
}

__global__ __launch_bounds__(1024) void topk_plan(
    const int64_t* __restrict__ kk, const uint32_t* __restrict__ fcount, const uint32_t* __restrict__ fhist,
    const uint32_t* __restrict__ bbase, int32_t* __restrict__ fbucket, uint32_t* __restrict__ bstart,
    BucketRec* __restrict__ brec, uint32_t* __restrict__ bfill, const int64_t* __restrict__ kb2,
    uint32_t* __restrict__ flag, uint32_t* __restrict__ status, const uint32_t* __restrict__ tkey,
    uint32_t* __restrict__ zcnt, int dbg, int32_t t0) {
  // (the verdict words in status are read by the kernels queued behind: the bucket kernels, the
  // zero fill and the exact tail — no host round trip)
  topk_plan_tensor((int)(t0 + blockIdx.x), kk, fcount, fhist, bbase, fbucket, bstart, brec, bfill, kb2, flag, status,
                   tkey, zcnt, dbg);
}

// Fast path, scatter: every kept candidate into its bucket (rank window of the tensor's
// region kb2[t] of the bucket buffer).  Per super-item: LDS counts per bucket, one global
// reservation per touched bucket, then LDS ranks.  Order inside a bucket is arbitrary (the
// bucket sort orders by the full key).
// SMALL (every tensor of the launch has <= kScatterSmallB bucket slots): the tensor's bucket
// table is staged in LDS as 16-bit entries, so the per-key bucket lookup is an LDS read instead
// of a global load that waits on the key load (two such round trips per key otherwise).
#ifndef OMF_SCATTER_CACHE  // key loads per thread (x4) kept in registers between the two phases
#define OMF_SCATTER_CACHE 3
#endif
template <bool SMALL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void topk_bucket_scatter(
    const uint64_t* __restrict__ cand, const Item* __restrict__ items, const uint32_t* __restrict__ sub_cnt,
    const uint4* __restrict__ supinfo, const uint32_t* __restrict__ fmap, const uint32_t* __restrict__ tlo,
    const uint32_t* __restrict__ fcount, const int32_t* __restrict__ fbucket, const uint32_t* __restrict__ bbase,
    const uint32_t* __restrict__ bstart, uint32_t* __restrict__ bfill, const int64_t* __restrict__ kb2,
    const int64_t* __restrict__ tbegin, float* __restrict__ r, uint64_t* __restrict__ bkeys,
    const uint32_t* __restrict__ status, const uint32_t* __restrict__ thi, uint32_t sup0) {
  if (status[1] | status[2]) return;  // the plan's verdict is a fallback: nothing to do
  __shared__ uint32_t s_b[SMALL ? kScatterSmallB : kPlanMaxBuckets];
  __shared__ int16_t s_fb[SMALL ? kFineMax : 1];
  __shared__ uint32_t s_spre[1025], s_part[1024];
  __shared__ int64_t s_ibeg[kSupItems];
  __shared__ uint32_t s_map[kCoarse];
  SupView v{s_spre, s_ibeg, 0, 0, false};
  v.init(supinfo, items, sub_cnt, fmap, s_map, s_part, sup0 + blockIdx.x);
  const int t = v.t;
  const uint32_t lo = tlo[t], F = fcount[t], b0 = bbase[t], nb = bbase[t + 1] - b0, hi = thi[t];
  const int64_t base = tbegin[t];
  const uint32_t nbl = SMALL ? nb : min(nb, (uint32_t)kPlanMaxBuckets);  // topk_plan's buckets are < nbl
  for (uint32_t j = threadIdx.x; j < nbl; j += 1024) s_b[j] = 0;
  const uint32_t* map_t = s_map;
  const int32_t* fb = fbucket + (size_t)t * kFineMax;
  if (SMALL)
    for (uint32_t j = threadIdx.x; j < F; j += 1024) s_fb[j] = (int16_t)fb[j];
  __syncthreads();
  constexpr int U = 4;
  // SMALL: the first CI x U keys of each thread (and their buckets) stay in registers from the
  // count phase to the place phase, so most keys are read from memory once, not twice
  constexpr int CI = SMALL ? OMF_SCATTER_CACHE : 0;
  uint64_t* dst = bkeys + kb2[t];
  const auto load = [&](uint32_t e0, uint64_t (&key)[U], int32_t (&j)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t e = min(e0 + (uint32_t)u * 1024, v.total - 1);
      key[u] = cand[v.pos(e)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t f = fine_bin((uint32_t)key[u] & 0x7fffffffu, lo, map_t, F);
      j[u] = SMALL ? (int32_t)s_fb[f] : fb[f];
    }
  };
  const auto visit = [&](int phase, uint32_t e0, const uint64_t (&key)[U], const int32_t (&j)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e0 + (uint32_t)u * 1024 >= v.total) continue;
      if (j[u] < 0) {  // below the k-th key's bin: not selected (a "sure" key gets its t' back)
        if (phase == 1 && r && ((uint32_t)key[u] & 0x7fffffffu) >= hi)
          r[base + (key[u] >> 32)] = __uint_as_float((uint32_t)key[u]);
        continue;
      }
      if (phase == 0) {
        atomicAdd(&s_b[j[u]], 1u);
      } else {
        const uint32_t p = atomicAdd(&s_b[j[u]], 1u);
        dst[p] = key[u];
      }
    }
  };
  uint64_t ck[CI > 0 ? CI : 1][U];
  int32_t cj[CI > 0 ? CI : 1][U];
#pragma unroll
  for (int i = 0; i < CI; ++i)
    if (threadIdx.x + (uint32_t)i * U * 1024 < v.total) load(threadIdx.x + (uint32_t)i * U * 1024, ck[i], cj[i]);
  for (int phase = 0; phase < 2; ++phase) {  // 0: count per bucket; 1: place
#pragma unroll
    for (int i = 0; i < CI; ++i)
      if (threadIdx.x + (uint32_t)i * U * 1024 < v.total) visit(phase, threadIdx.x + (uint32_t)i * U * 1024, ck[i], cj[i]);
    for (uint32_t e0 = threadIdx.x + (uint32_t)CI * U * 1024; e0 < v.total; e0 += U * 1024) {
      uint64_t key[U];
      int32_t j[U];
      load(e0, key, j);
      visit(phase, e0, key, j);
    }
    __syncthreads();
    if (phase == 0) {  // reserve each touched bucket's range; s_b := this block's first slot
      for (uint32_t q = threadIdx.x; q < nbl; q += 1024)
        if (s_b[q]) s_b[q] = bstart[b0 + q] + atomicAdd(&bfill[b0 + q], s_b[q]);
      __syncthreads();
    }
  }
}

// Fast path, one block per bucket: order its <= 2 kBucketHalf keys by (|t'| descending, index
// ascending) in LDS and write the ranks below k: values, int64 indices, and (error feedback)
// zero the selected residual slots.  Ordering is a counting sort on 4096 sub-bins that split
// the bucket's |t'| range evenly (about one key per sub-bin), then an insertion sort inside
// each sub-bin; a bucket with a sub-bin of more than kMaxRun keys (ties, clusters) is merge
// sorted instead.  Sort key: (2^31-1-|t'|bits) << 33 | index << 1 | sign.
constexpr int kSubBins = kBT * kBI;  // 4096
constexpr uint32_t kMaxRun = 32;
#ifndef OMF_SORT_WAVES  // waves per SIMD the bucket sort is compiled for (experiment builds may override)
#define OMF_SORT_WAVES 6
#endif
__global__ __launch_bounds__(kBT) __attribute__((amdgpu_waves_per_eu(OMF_SORT_WAVES))) void topk_bucket_sort(
    const uint64_t* __restrict__ bkeys, const BucketRec* __restrict__ brec, const int64_t* __restrict__ kk,
    const int64_t* __restrict__ koff, const int64_t* __restrict__ tbegin, const int64_t* __restrict__ tsize,
    float* __restrict__ r, float* __restrict__ values, int64_t* __restrict__ indices,
    const uint32_t* __restrict__ status, const uint32_t* __restrict__ thi, int dbg, uint32_t b0) {
  // 40 KiB of LDS (four blocks per CU): the sub-bin counters, then offsets, are 16-bit fields
  // packed two per word (a bucket holds <= 4096 keys), and the scan's wave totals borrow the first
  // words of that array while it holds nothing live.
  __shared__ union {
    uint64_t xch[kSubBins];
    struct {
      uint64_t out[kSubBins];
      uint32_t start2[kSubBins / 2];
    } cs;
    struct {  // the level-1 histogram, and the wave min / max (then scan totals)
      uint32_t h1[kBT];
      uint32_t mm[2 * (kBT / 64)];
    } lv;
  } s_u;
  const BucketRec rec = brec[b0 + blockIdx.x];
  const uint32_t cnt = rec.count_tensor & 0xffffu;
  if (cnt == 0 || (status[1] | status[2])) return;  // block-uniform (a fallback verdict: nothing to do)
  const int t = (int)(rec.count_tensor >> 16);
  const uint32_t st = rec.start;
  const uint64_t* src = bkeys + rec.key_off;
  const int64_t k = kk[t], o = koff[t], base = tbegin[t], n = tsize[t];  // issued with the key loads
  uint64_t keys[kBI];
  uint32_t meta[kBI];  // sub-bin << 16 | slot in it (0xffffffff: no key)
  // Sub-bin of a key from the bucket's own keys, in LDS (no memory round after the key loads):
  // the bucket's |t'| range [mmin, mmax] is cut into kBT equal level-1 bins, counted and scanned;
  // a key's sub-bin = its level-1 bin's first rank plus its linear position inside that bin times
  // the bin's count — about one key per sub-bin, monotone in |t'| (descending), so the counting
  // sort below plus an insertion sort per sub-bin orders the bucket exactly.
  const uint32_t hi = thi[t];
#pragma unroll
  for (int j = 0; j < kBI; ++j) keys[j] = src[min(threadIdx.x + (uint32_t)j * kBT, cnt - 1u)];  // striped
  uint32_t mn = 0xffffffffu, mx = 0u;
#pragma unroll
  for (int j = 0; j < kBI; ++j) {  // past the count: the last key again (no effect on the range)
    const uint32_t mag = (uint32_t)keys[j] & 0x7fffffffu;
    mn = min(mn, mag);
    mx = max(mx, mag);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor(mn, d, 64));
    mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_u.lv.mm[wave] = mn;
    s_u.lv.mm[kBT / 64 + wave] = mx;
  }
  s_u.lv.h1[threadIdx.x] = 0;
  for (int i = threadIdx.x; i < kSubBins / 2; i += kBT) s_u.cs.start2[i] = 0;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kBT / 64; ++w) {
    mn = min(mn, s_u.lv.mm[w]);
    mx = max(mx, s_u.lv.mm[kBT / 64 + w]);
  }
  // y = (mmax - |t'|) * kBT / range: one rounding of a monotone product, so monotone in |t'|
  const float sc = (float)kBT / (float)((uint64_t)mx - mn + 1u);
  float y[kBI];
  uint32_t b1[kBI];
#pragma unroll
  for (int j = 0; j < kBI; ++j) {
    y[j] = (float)(mx - ((uint32_t)keys[j] & 0x7fffffffu)) * sc;
    b1[j] = min((uint32_t)y[j], (uint32_t)kBT - 1u);
    if (threadIdx.x + (uint32_t)j * kBT < cnt) atomicAdd(&s_u.lv.h1[b1[j]], 1u);
  }
  __syncthreads();
  {
    const uint32_t c1 = s_u.lv.h1[threadIdx.x];
    uint32_t tot;
    const uint32_t inc = block_scan_incl<kBT>(c1, s_u.lv.mm, tot);  // begins with a barrier
    s_u.lv.h1[threadIdx.x] = (inc - c1) | (c1 << 16);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kBI; ++j) {
    const uint32_t e = threadIdx.x + (uint32_t)j * kBT;
    const uint32_t w = s_u.lv.h1[b1[j]], c = w >> 16;
    const uint32_t in = min((uint32_t)((y[j] - (float)b1[j]) * (float)c), c - 1u);
    const uint32_t bits = (uint32_t)keys[j], mag = bits & 0x7fffffffu;
    meta[j] = e < cnt ? min((w & 0xffffu) + in, cnt - 1u) : 0xffffffffu;
    keys[j] = e < cnt ? ((uint64_t)(0x7fffffffu - mag) << 33) | ((keys[j] >> 32) << 1) | (uint64_t)(bits >> 31) : ~0ull;
  }
#pragma unroll
  for (int j = 0; j < kBI; ++j) {
    if (meta[j] == 0xffffffffu) continue;
    const uint32_t sb = meta[j], sh = 16u * (sb & 1u);
    meta[j] = (sb << 16) | ((atomicAdd(&s_u.cs.start2[sb >> 1], 1u << sh) >> sh) & 0xffffu);
  }
  __syncthreads();
  uint32_t c[kBI], loc = 0, over = 0;  // this thread's sub-bins kBI tid ..
#pragma unroll
  for (int j = 0; j < kBI; j += 2) {
    const uint32_t w2 = s_u.cs.start2[(threadIdx.x * kBI + j) >> 1];
    c[j] = w2 & 0xffffu;
    c[j + 1] = w2 >> 16;
    loc += c[j] + c[j + 1];
    over |= (c[j] > kMaxRun || c[j + 1] > kMaxRun) ? 1u : 0u;
  }
  // one scan carries both the counts (< 2^20) and, above them, how many threads saw a sub-bin
  // of more than kMaxRun keys; its first barrier orders every thread's reads of start2 before
  // the wave totals land there
  uint32_t tot;
  const uint32_t inc = block_scan_incl<kBT>(loc | (over << 20), s_u.cs.start2, tot) & 0xfffffu;
  const bool merge = (tot >> 20) != 0u;  // block-uniform
  __syncthreads();  // every thread has read the wave totals
  if (!merge && !(dbg & 1)) {
    uint32_t run = inc - loc;
#pragma unroll
    for (int j = 0; j < kBI; j += 2) {
      s_u.cs.start2[(threadIdx.x * kBI + j) >> 1] = run | ((run + c[j]) << 16);
      run += c[j] + c[j + 1];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kBI; ++j)
      if (meta[j] != 0xffffffffu) {
        const uint32_t sb = meta[j] >> 16;
        const uint32_t at = (s_u.cs.start2[sb >> 1] >> (16u * (sb & 1u))) & 0xffffu;
        s_u.cs.out[at + (meta[j] & 0xffffu)] = keys[j];
      }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kBI; ++j) {  // insertion sort inside each sub-bin
      if (c[j] < 2) continue;
      const uint32_t sb = threadIdx.x * kBI + j;
      uint64_t* a = s_u.cs.out + ((s_u.cs.start2[sb >> 1] >> (16u * (sb & 1u))) & 0xffffu);
      for (uint32_t x = 1; x < c[j]; ++x) {
        const uint64_t v = a[x];
        uint32_t y = x;
        for (; y > 0 && a[y - 1] > v; --y) a[y] = a[y - 1];
        a[y] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kBI; ++j) keys[j] = s_u.cs.out[threadIdx.x + j * kBT];
  } else if (merge) {  // rare (ties, clusters): a bitonic sort of the whole bucket in LDS
#pragma unroll
    for (int j = 0; j < kBI; ++j) s_u.xch[threadIdx.x + j * kBT] = keys[j];  // no key: ~0, sorts last
    __syncthreads();
#pragma unroll 1
    for (uint32_t size = 2; size <= (uint32_t)kSubBins; size <<= 1)
#pragma unroll 1
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll 1
        for (uint32_t i = threadIdx.x; i < (uint32_t)kSubBins / 2; i += kBT) {
          const uint32_t a = 2 * i - (i & (stride - 1)), b = a + stride;  // a: bit `stride` clear
          const uint64_t ka = s_u.xch[a], kb = s_u.xch[b];
          if ((ka > kb) == ((a & size) == 0)) {  // ascending where bit `size` of a is clear
            s_u.xch[a] = kb;
            s_u.xch[b] = ka;
          }
        }
        __syncthreads();
      }
#pragma unroll
    for (int j = 0; j < kBI; ++j) keys[j] = s_u.xch[threadIdx.x + j * kBT];
  }
#pragma unroll
  for (int j = 0; j < kBI; ++j) {
    const uint32_t p = threadIdx.x + (uint32_t)j * kBT;
    if (p >= cnt) break;
    const int64_t rank = (int64_t)st + p;
    const uint64_t sk = keys[j];
    const uint32_t idx = (uint32_t)(sk >> 1) & 0x3ffffffu;
    if ((int64_t)idx >= n) continue;  // never expected (a padding key inside the bucket's count)
    const float v = __uint_as_float(((uint32_t)(sk & 1u) << 31) | (0x7fffffffu - (uint32_t)(sk >> 33)));
    const bool sure = (0x7fffffffu - (uint32_t)(sk >> 33)) >= hi;
    if (rank < k) {
      values[o + rank] = v;
      indices[o + rank] = (int64_t)idx;
      if (r && !sure && !(dbg & 2)) r[base + idx] = __fsub_rn(v, v);  // selected below the sure bin
    } else if (r && sure && !(dbg & 2)) {
      r[base + idx] = v;  // a "sure" key that was not selected after all: t' back
    }
  }
}

// Fast path, plan + scatter in one launch (every tensor of the launch with <= kScatterSmallB bucket
// slots; the LDS sort, which needs no fine-bin ranks): each super-item block plans its own tensor's
// buckets in LDS from the exact fine-bin histogram — the counts (16 per thread), one block scan, the
// bucket of every kept bin and each bucket's first rank — exactly as topk_plan_tensor, so the bucket
// table and the buckets' first ranks never go through global memory and no launch (with its drain)
// separates the plan from the scatter.  The tensor's first super-item block also writes the bucket
// records, the zero-fill count and the redo flag, sets the verdict bits, and arrives on the call's
// counter (one arrival per tensor, as topk_plan's blocks): the last tensor to arrive publishes the
// verdict to mapped host memory early in the launch.  A block whose own tensor is flagged (redo, or a
// fine bin over kBucketHalf keys, whose keys could run past the tensor's bucket region) places
// nothing: the call takes the fallback, which restores every candidate's residual.  Blocks of
// unflagged tensors proceed whatever the others' verdicts (their bucket writes are then unused).
#ifndef OMF_PLANNED_CACHE  // key loads per thread (x4) kept in registers between the scatter's phases
#define OMF_PLANNED_CACHE 2
#endif
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void topk_scatter_planned(
    const uint64_t* __restrict__ cand, const Item* __restrict__ items, const uint32_t* __restrict__ sub_cnt,
    const uint4* __restrict__ supinfo, const uint32_t* __restrict__ fmap, const uint32_t* __restrict__ tlo,
    const uint32_t* __restrict__ fcount, const uint32_t* __restrict__ fhist, const int64_t* __restrict__ kk,
    const uint32_t* __restrict__ tkey, const uint32_t* __restrict__ bbase, BucketRec* __restrict__ brec,
    uint32_t* __restrict__ bfill, const int64_t* __restrict__ kb2, const int64_t* __restrict__ tbegin,
    float* __restrict__ r, uint64_t* __restrict__ bkeys, uint32_t* __restrict__ flag, uint32_t* __restrict__ zcnt,
    uint32_t* __restrict__ status, const uint32_t* __restrict__ thi, uint32_t sup0) {
  __shared__ uint32_t s_b[kScatterSmallB];   // per bucket: this block's count, then its first slot
  __shared__ uint32_t s_bs[kScatterSmallB];  // per bucket: its first rank in the tensor
  __shared__ int16_t s_fb[kFineMax];         // per fine bin: its bucket (-1: below the k-th key's bin)
  __shared__ uint32_t s_spre[1025], s_part[1024];
  __shared__ int64_t s_ibeg[kSupItems];
  __shared__ uint32_t s_map[kCoarse];
  __shared__ uint32_t s_kend, s_nb, s_over, s_nbig;
  __shared__ uint32_t s_big[kMaxBigBins];    // first ranks of the kept big fine bins
  SupView v{s_spre, s_ibeg, 0, 0, false};
  v.init(supinfo, items, sub_cnt, fmap, s_map, s_part, sup0 + blockIdx.x);
  const int t = v.t;
  const uint32_t lo = tlo[t], F = fcount[t], b0 = bbase[t], nbmax = bbase[t + 1] - b0, hi = thi[t];
  const int64_t base = tbegin[t];
  // ---- the plan (topk_plan_tensor's rule)
  constexpr int PER = kFineMax / 1024;
  const uint32_t* ht = fhist + (size_t)t * kFineMax;
  uint32_t h[PER], loc = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const uint32_t i = PER * threadIdx.x + j;
    h[j] = i < F ? ht[i] : 0u;
    loc += h[j];
  }
  if (threadIdx.x == 0) {
    s_kend = 0;
    s_nb = 0;
    s_over = 0;
    s_nbig = 0;
  }
  for (uint32_t j = threadIdx.x; j < nbmax; j += 1024) {
    s_bs[j] = 0xffffffffu;
    s_b[j] = 0;
  }
  uint32_t tot32;
  const uint32_t inc = block_scan_incl<1024>(loc, s_part, tot32);  // begins with a barrier
  const bool zero_mode = tkey[t] == 1u;
  uint32_t k = (uint32_t)kk[t];  // (k <= n <= 2^25)
  const bool redo = tot32 < k && !zero_mode;  // the sampled threshold was too high: exact redo
  const bool zero_fill = tot32 < k && zero_mode;  // every candidate selected, then zeros
  if (zero_fill) k = tot32;
  // Big fine bins (> kBucketHalf keys, up to 2 kBucketHalf) get a bucket of their own: bin i goes to
  // bucket floor(se_i / kBucketHalf) + B_i + big_i, B_i = kept big bins above it, so every other
  // bucket still holds the bins whose rank starts fall in one kBucketHalf window (<= 2 kBucketHalf
  // keys) and a big bin's bucket holds it alone.  The kept big bins' first ranks go to an LDS list
  // (rare: usually empty) that each bin counts below its own.  Only a bin of more than 2 kBucketHalf
  // keys (one magnitude key shared that widely, a cluster the fine bins cannot split), or more than
  // kMaxBigBins of them, takes the fallback.
  if (!redo) {
    uint32_t se = tot32 - inc;  // keys in the bins of higher threads
#pragma unroll
    for (int j = PER - 1; j >= 0; --j) {
      if (h[j] > (uint32_t)kBucketHalf && se < k) {
        const uint32_t q = atomicAdd(&s_nbig, 1u);
        if (q < (uint32_t)kMaxBigBins) s_big[q] = se;
      }
      se += h[j];
    }
  }
  __syncthreads();
  const uint32_t nbig = s_nbig;
  if (!redo) {
    uint32_t se = tot32 - inc;
#pragma unroll
    for (int j = PER - 1; j >= 0; --j) {
      const uint32_t i = PER * threadIdx.x + j;
      int32_t bucket = -1;
      if (h[j] && se < k) {
        uint32_t above = 0;
        for (uint32_t q = 0; q < min(nbig, (uint32_t)kMaxBigBins); ++q) above += s_big[q] < se ? 1u : 0u;
        bucket = (int32_t)(se / kBucketHalf + above + (h[j] > (uint32_t)kBucketHalf ? 1u : 0u));
        if (nbig > (uint32_t)kMaxBigBins || (uint32_t)bucket >= nbmax || h[j] > (uint32_t)kBucketPad) {
          s_over = 1u;  // a bin the bucket sort cannot hold (or too many big ones)
          bucket = -1;
        } else {
          atomicMin(&s_bs[bucket], se);
          if (v.first) atomicAdd(&s_b[bucket], h[j]);  // the bucket's key count, for its record
          if (se + h[j] >= k) {  // the bin of the k-th key (exactly one)
            s_kend = se + h[j];
            s_nb = (uint32_t)bucket + 1u;
          }
        }
      }
      if (i < F) s_fb[i] = (int16_t)bucket;
      se += h[j];
    }
  }
  __syncthreads();
  const bool skip = redo || s_over != 0u;  // block-uniform
  if (v.first) {  // the tensor's records, flags and verdict bits
    const uint32_t nb = s_nb;
    for (uint32_t j = threadIdx.x; j < nbmax; j += 1024) {
      uint32_t st = 0, c = 0;
      if (!skip && j < nb && s_bs[j] != 0xffffffffu) {
        st = s_bs[j];
        c = s_b[j];
      }
      brec[b0 + j] = BucketRec{(uint64_t)kb2[t] + st, st, min(c, 0xffffu) | ((uint32_t)t << 16)};
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nbmax; j += 1024) s_b[j] = 0;  // this block's per-bucket counts next
    if (threadIdx.x == 0) {
      flag[t] = redo ? 1u : 0u;
      zcnt[t] = zero_fill ? tot32 : kNoZeroFill;
      if (redo) atomicOr(&status[1], 1u);
      if (!redo && s_over) atomicOr(&status[2], 1u);
      if (zero_fill) atomicOr(&status[0], 1u);
    }
  }
  if (skip) return;
  if (v.first) __syncthreads();  // (its s_b cleared)
  // ---- the scatter (topk_bucket_scatter<true> with the LDS plan)
  const uint32_t* map_t = s_map;
  uint64_t* dst = bkeys + kb2[t];
  constexpr int U = 4;
  constexpr int CI = OMF_PLANNED_CACHE;
  const auto load = [&](uint32_t e0, uint64_t (&key)[U], int32_t (&j)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t e = min(e0 + (uint32_t)u * 1024, v.total - 1);
      key[u] = cand[v.pos(e)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) j[u] = (int32_t)s_fb[fine_bin((uint32_t)key[u] & 0x7fffffffu, lo, map_t, F)];
  };
  const auto visit = [&](int phase, uint32_t e0, const uint64_t (&key)[U], const int32_t (&j)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e0 + (uint32_t)u * 1024 >= v.total) continue;
      if (j[u] < 0) {  // below the k-th key's bin: not selected (a "sure" key gets its t' back)
        if (phase == 1 && r && ((uint32_t)key[u] & 0x7fffffffu) >= hi)
          r[base + (key[u] >> 32)] = __uint_as_float((uint32_t)key[u]);
        continue;
      }
      if (phase == 0) {
        atomicAdd(&s_b[j[u]], 1u);
      } else {
        const uint32_t p = atomicAdd(&s_b[j[u]], 1u);
        dst[p] = key[u];
      }
    }
  };
  uint64_t ck[CI > 0 ? CI : 1][U];
  int32_t cj[CI > 0 ? CI : 1][U];
#pragma unroll
  for (int i = 0; i < CI; ++i)
    if (threadIdx.x + (uint32_t)i * U * 1024 < v.total) load(threadIdx.x + (uint32_t)i * U * 1024, ck[i], cj[i]);
  for (int phase = 0; phase < 2; ++phase) {  // 0: count per bucket; 1: place
#pragma unroll
    for (int i = 0; i < CI; ++i)
      if (threadIdx.x + (uint32_t)i * U * 1024 < v.total) visit(phase, threadIdx.x + (uint32_t)i * U * 1024, ck[i], cj[i]);
    for (uint32_t e0 = threadIdx.x + (uint32_t)CI * U * 1024; e0 < v.total; e0 += U * 1024) {
      uint64_t key[U];
      int32_t j[U];
      load(e0, key, j);
      visit(phase, e0, key, j);
    }
    __syncthreads();
    if (phase == 0) {  // reserve each touched bucket's range; s_b := this block's first slot
      for (uint32_t q = threadIdx.x; q < nbmax; q += 1024)
        if (s_b[q]) s_b[q] = s_bs[q] + atomicAdd(&bfill[b0 + q], s_b[q]);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- host side: a call's groups
// Per host thread and device: the group pipeline's second stream and its events (made on first
// use; experiment builds only use more than one group).
struct HostSync {
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t fused[2] = {nullptr, nullptr};  // per stream: its latest group's streaming pass issued
};
HostSync* host_sync(int dev) {
  constexpr int kMaxDev = 64;
  thread_local HostSync hs[kMaxDev];
  if (dev < 0 || dev >= kMaxDev) return nullptr;
  return &hs[dev];
}

// The second stream and the fork / join events of the group pipeline (per device and thread).
int pipe_streams(HostSync* h) {
  if (h->side) return OMF_OK;
  OMF_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
  for (hipEvent_t* e : {&h->fork, &h->join, &h->fused[0], &h->fused[1]})
    OMF_HIP(hipEventCreateWithFlags(e, kOrderEventFlags));
  return OMF_OK;
}

// Pipeline groups of the sampled path (topk_layout::make_groups): each group's chain (sample -> fused
// pass -> fine histogram -> plan -> bucket scatter -> bucket sort) is one run of launches on one of two
// streams, alternating, so that one group's latency-bound kernels (the last sample blocks, the
// per-tensor plans, the bucket sorts) run beside the next group's streaming pass instead of after the
// whole arena's.
int topk_group_count(const omf_plan* p, const TopkKnobs& kn) {
  // Off by default: measured on Llama-400M more groups only add time —
  // 1.089 ms with one group, 1.156 / 1.192 / 1.266 ms with 2 / 3 / 4 (the latency-bound kernels
  // do not shrink with their group, and their random stores slow the streaming pass beside them).
  int g = kn.groups;
  if (p->arena_end < ((int64_t)1 << 24)) g = 1;  // small arenas: launch-bound
  return std::max(1, std::min(g, std::min(16, p->nt)));
}

}  // namespace

int omf::topk_launch_sampled(const TopkCall& c, int64_t max_runs, float2 sure_zc) {  // omf_topk_enc.h
  const omf_plan* plan = c.plan;
  const TopkKnobs& kn = plan->topk_knobs;
  const EncodeWs& w = c.w;
  const SetupTable& tb = c.tb;
  const Item* items = plan->d_flat;
  const int64_t *d_sizes = plan->d_sizes, *d_begins = plan->d_begins;
  hipStream_t st = c.st;
  HostSync* hsync = host_sync(plan->device);
  if (!hsync) return fail(OMF_EHIP, "omf_topk_encode: device index out of range");
  const bool forced = kn.force_fallback != 0;
  const std::vector<Group> groups = make_groups(*c.host, topk_group_count(plan, kn));
  if (groups.size() > 1)
    if (int r = pipe_streams(hsync)) return r;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const Group& G = groups[gi];
    // group 0 runs on the caller's stream; its sample launch (which clears the call's status
    // words) is the fork point of the second stream
    hipStream_t s = (gi & 1) ? hsync->side : st;
    const dim3 sblk(1024);
    if (G.nsb)
      hipLaunchKernelGGL(c.mode == 1 ? topk_sample<1> : topk_sample<0>, dim3(G.nsb), sblk, 0, s, c.x, c.residual,
                         c.alpha, d_begins, d_sizes, (const uint32_t*)tb.smap, max_runs, tb.gh, tb.gz, tb.arrive,
                         w.status, tb.kk, tb.tfirst, tb.tlast, w.tkey, w.hist, w.item_cnt, w.thi, w.fmap, w.tlo,
                         w.fcount, w.fhist, G.sb0, sure_zc);
    if (gi == 0 && groups.size() > 1) {
      OMF_HIP(hipEventRecord(hsync->fork, st));
      OMF_HIP(hipStreamWaitEvent(hsync->side, hsync->fork, 0));
    }
    // The streaming passes run one after another: group g's waits for group g-1's (on the
    // other stream), so that g-1's latency-bound tail (fine histogram, plan, bucket kernels)
    // runs beside g's streaming pass rather than two passes sharing the memory system.
    if (gi > 0) OMF_HIP(hipStreamWaitEvent(s, hsync->fused[(gi - 1) & 1], 0));
    const dim3 fgrid(G.nsub);
    hipLaunchKernelGGL(c.mode == 1 ? topk_fused<1> : c.mode == 2 ? topk_fused<2> : topk_fused<0>, fgrid,
                       dim3(kSubThreads), 0, s, c.x, c.residual, c.alpha, items, d_begins, w.tkey, w.thi, w.sub_cnt,
                       w.item_cnt, w.cand, G.sub0);
    if (groups.size() > 1) OMF_HIP(hipEventRecord(hsync->fused[gi & 1], s));
    // fast path: exact fine-bin histograms, bucket plan
    const dim3 supgrid(G.nsup), supblk(1024);
    hipLaunchKernelGGL(topk_fine_hist, supgrid, supblk, 0, s, w.cand, items, w.sub_cnt, (const uint4*)tb.supinfo, w.fmap,
                       w.tlo, w.fcount, w.fhist, tb.bbase, w.bfill, G.sup0);
    // the plan writes the verdict words (status); the bucket kernels behind it do nothing on a
    // fallback verdict, which the exact tail then handles
    const bool small = G.nb_max <= kScatterSmallB && kn.scatter_small;
    if (!forced && small && kn.planned_scatter)  // the plan inside the scatter launch
      hipLaunchKernelGGL(topk_scatter_planned, supgrid, supblk, 0, s, w.cand, items, w.sub_cnt,
                         (const uint4*)tb.supinfo, w.fmap, w.tlo, w.fcount, w.fhist, tb.kk, w.tkey, tb.bbase, w.brec,
                         w.bfill, tb.kb2, d_begins, c.rz, w.sorted, w.flag, w.zcnt, w.status, w.thi, G.sup0);
    else
      hipLaunchKernelGGL(topk_plan, dim3((unsigned)(G.t1 - G.t0)), sblk, 0, s, tb.kk, w.fcount, w.fhist, tb.bbase,
                         w.fbucket, w.bstart, w.brec, w.bfill, tb.kb2, w.flag, w.status, w.tkey, w.zcnt, kn.dbg, G.t0);
    if (!forced) {
      if (!(small && kn.planned_scatter)) {  // (the planned scatter has run above)
        hipLaunchKernelGGL(small ? topk_bucket_scatter<true> : topk_bucket_scatter<false>, supgrid, supblk, 0, s,
                           w.cand, items, w.sub_cnt, (const uint4*)tb.supinfo, w.fmap, w.tlo, w.fcount, w.fbucket,
                           tb.bbase, w.bstart, w.bfill, tb.kb2, d_begins, c.rz, w.sorted, w.status, w.thi, G.sup0);
      }
      hipLaunchKernelGGL(topk_bucket_sort, dim3(G.nbk), dim3(kBT), 0, s, w.sorted, w.brec, tb.kk, tb.koff, d_begins,
                         d_sizes, c.rz, c.values, c.indices, w.status, w.thi, kn.dbg, G.bk0);
    }
    OMF_HIP(hipGetLastError());
  }
  if (groups.size() > 1) {  // join: the caller's stream continues after the second stream's work
    OMF_HIP(hipEventRecord(hsync->join, hsync->side));
    OMF_HIP(hipStreamWaitEvent(st, hsync->join, 0));
  }
  return OMF_OK;
}
