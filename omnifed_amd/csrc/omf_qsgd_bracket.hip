// omf_qsgd_bracket.hip — the bracketed single-read QSGD encoder (strategy 3), MI355X (gfx950).
//
// The default encoder from 2^25 elements.  Internal interface: omf_bracket.h; the device steps shared
// with the other encoders: omf_qsgd_enc.h; the element math: omf_qsgd_dev.h.
//
// Kernel map.  Strategy 3: x is read once without waiting for any norm.
//   qsgd_spec_bracket  one workgroup per tensor: a bracket [n_lo, n_hi] of its norm from a
//                      stratified sample (exact for small tensors) and the multipliers
//                      c_lo <= L / n_hi, c_hi >= L / n_lo (outward margins of 2^-20).
//   qsgd_spec_quant    one workgroup per 4 Ki-element block, no barrier: each wave's fp64
//                      partial sum of squares, and every element's level for ANY norm in the
//                      bracket: dl = fma(|x|, c_lo, -u), dh = fma(|x|, c_hi, -u); the level is
//                      ceil(dl) == ceil(dh) (clamped to L, sign of x) when they agree — the
//                      exact level is ceil(|RN(x/n)| L - u), monotone in n — else the quad is
//                      "undecided" and listed in the wave's slot (scripts/exp/spec_check.c
//                      checks the rule: 0 mismatches at brackets' end points and at decision
//                      points j + u; u == 0 with x != 0 is always undecided).
//   qsgd_spec_finish   its first workgroups fold the wave partials in segments (the last
//                      arriver folds the segments in order: the deterministic norm), check it
//                      lies in the bracket and publish {epoch, bad, norm}; the rest fix the
//                      listed quads exactly from their records (Markstein division, the shared
//                      element math), one thread per quad, polling their tensor's granule; a
//                      tensor whose norm fell outside its bracket, whose slots overflowed or
//                      whose sample was degenerate is requantised whole from x (the rare path).
//   qsgd_spec_bracket_wide  the bracket of wide levels (bit widths 5-8): kBrParts workgroups per tensor.
//   qsgd_spec_quant_fb, qsgd_spec_quant_wfb  the pass with the bracket folded in: its first workgroups
//                      are the bracket's parts (wfb: wide levels, one-wave workgroups).
// Payload bits equal every other strategy's for the same norm.  Each hand-off protocol has one copy:
// arrive_last / combine_parts (a tensor's parts or fold segments), fb_poll (the fused bracket's
// granules), spec_norm_wait (the norm's granule); fused_pass_block is the fused passes' block header.
//
// Host side (the end of the file): the two buffer groups made at the first encode that needs them,
// and omf::bracket::launch with its kernel tables.
#include <algorithm>
#include <cstdlib>

#include "omf_bracket.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_dec.h"
#include "omf_qsgd_dev.h"
#include "omf_qsgd_enc.h"

using namespace omf;
using namespace omf::plan_layout;  // the table records and layout constants (omf_plan_layout.h)

namespace {

constexpr int kSpecV = 4;                                    // float4 rows per thread
static_assert(kSpecBlk == (int64_t)kSpecV * kThreads * 4, "4096 elements per block");
// Wide levels (bit_width 5-8, fp32: the reference's default int32 wire at 8): the undecided fraction
// grows with L (a level step is norm / L wide), so a wave lists up to 32 quads (Llama-400M s = 8 with
// the sampled +-2.4 % brackets: ~10 per wave on its 1 Mi-element tensors, 2.1 M quads in all) and
// four fix threads share a wave slot.  Slots and records of this capacity are allocated at the
// plan's first wide encode.
constexpr int kSpecPerWaveWide = 32;
__host__ __device__ constexpr int spec_slot_words(int pw) { return pw == kSpecPerWave ? kSpecSlot : kWaves * pw; }
constexpr int64_t kSpecExact = 16384;                         // tensors read whole by the bracket
// (kSpecSlot, kSpecPerWave: omf_bracket.h; the sampled runs, the bracket parts, the fold segments and the
// bit widths served: omf_plan_layout.h; SpecBracket: omf_plan.h)

struct SpecArgs {
  EncArgs e;               // x, q, norm_out, items (flat 16 Ki items), alpha, levels, Philox key
  const int64_t* begins;   // per tensor
  const int64_t* sizes;
  const SpecBrItem* br_items;
  const SpecFoldItem* fold_items;
  SpecBracket* br;
  uint64_t* seg_part;      // per fold item: fp64 bits
  uint32_t* fold_cnt;      // per tensor arrival counters of the fold segments (reset by the last arriver)
  uint64_t* partials;      // fp64 bits, one per wave (kWaves per block)
  uint32_t* heads;         // per wave (dense, kWaves per block): (tensor << 8) | count of listed quads
  uint32_t* slots;         // spec_slot_words(PW) words per block: PW quad indices per wave
  float4* recs;            // per listed quad: its scaled x and its uniforms (2 float4), kWaves x PW per block
  uint32_t* flags;         // per tensor: a wave's slot overflowed (set by quant, cleared by fold)
  uint32_t* status;        // per tensor: 0 = listed quads only, 1 = requantise whole
  uint64_t* ngran;         // per tensor: {epoch << 1 | bad, norm} published by the fold
  uint64_t wait_ticks;     // bound of a fix thread's wait for its tensor's norm (100 MHz ticks)
  uint32_t dbg;            // test / experiment switches (omf_plan_set_debug spec bits 2-4), 0 in production
  float divisor;           // fused PS step: x := x / divisor (IEEE), written to xout; 0 = none
  float zsig;              // bracket half-width in standard deviations of the sample estimate (6)
  float* xout;
  uint32_t epoch;          // per-launch tag (never 0)
  uint32_t wide;           // wide levels: the bracket samples Rw runs (SpecBrItem), kBrParts workgroups per tensor
  double* br_part;         // wide / fused bracket: per (tensor, part) the partial {S1, S2}
  uint64_t* brgran;        // fused bracket: per tensor {epoch, c_lo} and {epoch, c_hi}
  uint32_t* br_cnt;        // wide: per tensor arrival counter (reset by the last arriver)
  int64_t nblocks;
  // Fused last-client decode-accumulate (omf_ps_accumulate_apply_encode; aq == NULL: none): before
  // the divide, x := fl32(x + fl32(fl32(anorm[t] * q) / alevels)) — the decoder's accumulate, bit
  // for bit (ainv = 2^-s for a power-of-two level count, else 0) — stored to aout when non-NULL.
  const void* aq;
  const float* anorm;
  float* aout;
  float alevels, ainv;
  int32_t awidth;          // 8 or 32: the last client's payload (LayerState.width)
};

// The last client's payload of one float4 row (AW = 1: int8, AW = 4: int32), loaded beside x.
template <int AW, bool FULL>
__device__ __forceinline__ int4 acc_load(const void* q, int64_t e, int64_t end) {
  if (AW == 1) {
    const int8_t* q8 = static_cast<const int8_t*>(q);
    if (FULL || e + 4 <= end)
      return make_int4(__builtin_nontemporal_load(reinterpret_cast<const int32_t*>(q8 + e)), 0, 0, 0);
    uint32_t w = 0;
    for (int c = 0; c < 3; ++c)
      if (e + c < end) w |= (uint32_t)(uint8_t)q8[e + c] << (8 * c);
    return make_int4((int32_t)w, 0, 0, 0);
  }
  const int32_t* q32 = static_cast<const int32_t*>(q);
  if (FULL || e + 4 <= end) {
    const i32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(q32 + e));
    return make_int4(t[0], t[1], t[2], t[3]);
  }
  int4 r = make_int4(0, 0, 0, 0);
  if (e < end) r.x = q32[e];
  if (e + 1 < end) r.y = q32[e + 1];
  if (e + 2 < end) r.z = q32[e + 2];
  return r;
}

// v + decode(raw): the decoders' element rule (qsgd_dec_elem, omf_qsgd_dec.h), as an accumulating decode.
template <int AW>
__device__ __forceinline__ float4 acc_add4(float4 v, int4 raw, float norm, float alevels, float ainv) {
  int32_t qi[4];
  if (AW == 1) {
    qsgd_split_i8(raw.x, qi);
  } else {
    qi[0] = raw.x; qi[1] = raw.y; qi[2] = raw.z; qi[3] = raw.w;
  }
  float y[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    y[c] = ainv != 0.0f ? qsgd_dec_elem<true>(norm, qi[c], alevels, ainv) : qsgd_dec_elem<false>(norm, qi[c], alevels, ainv);
  return make_float4(__fadd_rn(v.x, y[0]), __fadd_rn(v.y, y[1]), __fadd_rn(v.z, y[2]), __fadd_rn(v.w, y[3]));
}

// The bracket's view of one float4 of x at arena element e: x (+ the fused last client's decode).
__device__ __forceinline__ float4 br_value(const SpecArgs& a, float4 v, int64_t e, int64_t end, int32_t t) {
  if (!a.aq) return v;
  const float nrm = a.anorm[t];
  if (a.awidth == 32) return acc_add4<4>(v, acc_load<4, false>(a.aq, e, end), nrm, a.alevels, a.ainv);
  return acc_add4<1>(v, acc_load<1, false>(a.aq, e, end), nrm, a.alevels, a.ainv);
}

__device__ __forceinline__ uint32_t spec_hash(uint32_t a, uint32_t b) {
  uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return h;
}


__device__ __forceinline__ float4 scale_alpha(float4 v, float alpha) {
  if (alpha != 1.0f) {
    v.x = __fmul_rn(v.x, alpha); v.y = __fmul_rn(v.y, alpha);
    v.z = __fmul_rn(v.z, alpha); v.w = __fmul_rn(v.w, alpha);
  }
  return v;
}

// x * alpha (rounded to the value format when alpha != 1: torch.mul on a bf16 / fp16 tensor),
// then / divisor for the fused PS step (divisor 0: none) — the pass's arithmetic.
__device__ __forceinline__ float4 spec_prologue(float4 v, float alpha, float divisor, uint32_t fmt) {
  v = scale_alpha(v, alpha);
  if (fmt && alpha != 1.0f) v = round_fmt4(v, fmt);
  if (divisor != 0.0f) {
    v.x = __fdiv_rn(v.x, divisor); v.y = __fdiv_rn(v.y, divisor);
    v.z = __fdiv_rn(v.z, divisor); v.w = __fdiv_rn(v.w, divisor);
  }
  return v;
}


// ---------------------------------------------------------------- arrive last, combine in order
// A tensor's parts (of its bracket's sample, or the segments of its fold) hand their sums to the last
// of them to arrive, which combines them in part order: the same bits whichever part that is.  The
// hand-off is cdna_hip_programming.md §6 Guideline 16, one thread per part: the part's values stored
// sc1 and drained before the agent-scope add on the tensor's counter; the last arriver resets the
// counter for the next launch (relaxed: stream order) and reads the parts with sc1 loads.

// One thread: publish a part's N values in slot `slot` of row `row` of `all` (`parts` slots per row; the
// fold's segments are numbered through: row 0) and arrive at tensor t's counter; true in the last of `parts`.
template <int N>
__device__ __forceinline__ bool arrive_last(uint64_t* all, int32_t row, int64_t slot, const double (&v)[N],
                                            uint32_t* cnt, int32_t t, int parts) {
  uint64_t* mine = all + N * ((int64_t)row * parts + slot);
#pragma unroll
  for (int i = 0; i < N; ++i) st_agent(mine + i, (uint64_t)__double_as_longlong(v[i]));
  drain_vmem();
  const bool last = add_agent(&cnt[t], 1u) == (uint32_t)(parts - 1);
  if (last) __hip_atomic_store(&cnt[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return last;
}
// A workgroup: thread 0 arrives with the workgroup's values, every thread learns whether it was last.
template <int N>
__device__ __forceinline__ bool arrive_last_block(uint64_t* all, int32_t row, int64_t slot, const double (&v)[N],
                                                  uint32_t* cnt, int32_t t, int parts, uint32_t& s_last) {
  if (threadIdx.x == 0) s_last = arrive_last(all, row, slot, v, cnt, t, parts) ? 1u : 0u;
  __syncthreads();
  return s_last != 0u;
}
// The last arriver: the sums of the `parts` pairs {S1, S2} of row `row` of `all`, in part order.
__device__ __forceinline__ void combine_parts(const uint64_t* all, int32_t row, int parts, double (&S)[2]) {
  S[0] = S[1] = 0.0;
  for (int g = 0; g < parts; ++g) {
    const uint64_t* bp = all + 2 * ((int64_t)row * parts + g);
    S[0] += __longlong_as_double((long long)ld_agent(bp));
    S[1] += __longlong_as_double((long long)ld_agent(bp + 1));
  }
}

constexpr int kBrThreads = 1024;  // one bracket workgroup per tensor
constexpr int kBrWaves = kBrThreads / 64;

// Deterministic sum over a 1024-thread workgroup (wave butterflies, then the waves in order).
__device__ __forceinline__ double br_sum(double v, double* lds) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kBrWaves; ++w) s += lds[w];
  __syncthreads();
  return s;
}

// The bracket's sample of one tensor: runs of RUN elements at a hashed position inside each of R
// balanced strata (of >= 2 RUN elements); a run is RUN / 4 float4 loaded by consecutive lanes, 8
// passes per round (their loads in flight together); this workgroup takes the rounds part, part +
// parts, ...  Per run: s1 += its sum of squares, s2 += its square (in lane 0 of the run).
template <int RUN, bool AQ, int NT = kBrThreads, int PASSES = 8>
__device__ __forceinline__ void bracket_sample(const SpecArgs& a, const float* __restrict__ x, int32_t t, int64_t tb,
                                               int64_t n, int64_t R, int part, int parts, double& s1, double& s2) {
  constexpr int LPR = RUN / 4, RPP = NT / LPR, PER_ROUND = RPP * PASSES;
  const int64_t base = n / R, rem = n % R;
  const int j = threadIdx.x & (LPR - 1);
  const float alpha = a.e.alpha;
  for (int64_t rb = (int64_t)part * PER_ROUND; rb < R; rb += (int64_t)parts * PER_ROUND) {
    float4 v[PASSES];
    bool live[PASSES];
    auto run_pos = [&](int i) {  // element of this lane's float4 in pass i (recomputed: no VGPRs held)
      const int64_t r0 = rb + (int64_t)i * RPP + (threadIdx.x / LPR);
      const int64_t r = r0 < R ? r0 : 0;  // a dead lane re-reads run 0 (masked below)
      const int64_t lo = r * base + min(r, rem), len = base + (r < rem ? 1 : 0);
      return ((lo + (int64_t)(spec_hash((uint32_t)r, (uint32_t)t) % (uint32_t)(len - (RUN - 1)))) & ~(int64_t)3) + 4 * j;
    };
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      live[i] = rb + (int64_t)i * RPP + (threadIdx.x / LPR) < R;
      v[i] = *reinterpret_cast<const float4*>(x + run_pos(i));
    }
    if (AQ) {  // the fused PS step's last client (after every x load is issued)
#pragma unroll
      for (int i = 0; i < PASSES; ++i) v[i] = br_value(a, v[i], tb + run_pos(i), tb + n, t);
    }
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      float sr = live[i] ? sq4(spec_prologue(v[i], alpha, a.divisor, a.e.fmt), 0.0f) : 0.0f;
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) sr += __shfl_xor(sr, o, LPR);  // the run's sum in every lane
      if (live[i] && j == 0) {
        s1 += (double)sr;
        s2 += (double)sr * (double)sr;
      }
    }
  }
}

// WIDE: kBrParts workgroups per tensor, runs of kSpecRunWide (bit widths 5-8); AQ: the fused PS
// step's last client is added to the sample (narrow only).  One instance per case keeps each small
// enough for two 1024-thread workgroups per CU (one kernel for all three took 94 VGPRs).
__device__ SpecBracket bracket_from_sums(const SpecArgs& a, bool exact, int64_t n, int64_t R, int run, double S1,
                                         double S2);

template <bool WIDE, bool AQ>
__device__ __forceinline__ void spec_bracket_body(const SpecArgs& a, const SpecBrItem* __restrict__ items,
                                                  double* red, uint32_t& s_last) {
  // wide levels: kBrParts workgroups per tensor, part g sampling runs [g kSpecRuns, (g + 1) kSpecRuns)
  const int parts = WIDE ? kBrParts : 1;
  const int part = (int)(blockIdx.x % (unsigned)parts);
  const SpecBrItem bi = items[blockIdx.x / (unsigned)parts];  // one scalar load: the tensor's range and strata
  const int32_t t = bi.tensor;
  const int64_t tb = bi.begin, n = bi.n;
  const float* __restrict__ x = a.e.x + tb;
  const float alpha = a.e.alpha;
  double s1 = 0.0, s2 = 0.0;
  const bool exact = n <= kSpecExact;
  const int64_t R = WIDE ? (int64_t)bi.Rw : (int64_t)bi.R;
  // Loads are unconditional (a clamped address, the value masked after): a load under a
  // branch is waited for at the branch's end, which would serialise the round trips.
  if (exact) {  // 4 float4 per thread, all loads in flight
    constexpr int PER = (int)(kSpecExact / (4 * kBrThreads));
    float4 v[PER];
    const int64_t nq = n & ~(int64_t)3;  // whole quads
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t e = 4 * ((int64_t)i * kBrThreads + threadIdx.x);
      v[i] = nq ? *reinterpret_cast<const float4*>(x + (e < nq ? e : 0)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t e = 4 * ((int64_t)i * kBrThreads + threadIdx.x);
      if (e >= nq) {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < n) {  // the tensor's partial last quad (one thread)
          v[i].x = x[e];
          if (e + 1 < n) v[i].y = x[e + 1];
          if (e + 2 < n) v[i].z = x[e + 2];
        }
      }
    }
    if (AQ) {  // the fused PS step's last client, added before the divide
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int64_t e = 4 * ((int64_t)i * kBrThreads + threadIdx.x);
        if (e < n) v[i] = br_value(a, v[i], tb + e, tb + n, t);
      }
    }
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < PER; ++i) acc = sq4(spec_prologue(v[i], alpha, a.divisor, a.e.fmt), acc);
    s1 = acc;
  } else {
    bracket_sample<WIDE ? kSpecRunWide : kSpecRun, AQ>(a, x, t, tb, n, R, part, parts, s1, s2);
  }
  if (exact && part != 0) return;  // an exact tensor is one workgroup's
  double S[2];
  S[0] = br_sum(s1, red);
  S[1] = br_sum(s2, red);
  if (!exact && parts > 1) {  // the last part to arrive combines the partials in part order
    uint64_t* bp = reinterpret_cast<uint64_t*>(a.br_part);
    if (!arrive_last_block(bp, t, part, S, a.br_cnt, t, parts, s_last) || threadIdx.x != 0) return;
    combine_parts(bp, t, parts, S);
  }
  if (threadIdx.x != 0) return;
  a.br[t] = bracket_from_sums(a, exact, n, R, WIDE ? kSpecRunWide : kSpecRun, S[0], S[1]);
}

// The bracket of a tensor from its sample's sums (exact: S1 is the whole tensor's sum of squares).
__device__ SpecBracket bracket_from_sums(const SpecArgs& a, bool exact, int64_t n, int64_t R, int run, double S1,
                                         double S2) {
  double ss, k;
  if (exact) {
    ss = S1;
    k = 0x1p-12;  // fp32 per-thread accumulation differs from the fold's grouping
  } else {
    const double Rd = (double)R, m = S1 / Rd;
    const double var = fmax(0.0, (S2 - Rd * m * m) / (Rd - 1.0));
    ss = S1 * ((double)n / ((double)run * Rd));
    k = (double)a.zsig * sqrt(var / Rd) / m + 0x1p-10;  // 6 sigma of the run-sum estimate + 0.1 %
  }
  // bf16 / fp16 values: the norm is rounded to the format (at most half an ulp: 2^-8 / 2^-11
  // relative, so (1 + 2^-8)^2 < 1 + 2^-7 + 2^-14 on its square), and so is x / n, whose
  // rounding the multipliers absorb by the same relative bound (spec_quad_fmt).
  const uint32_t fmt = a.e.fmt;
  const double kf = fmt == kFmtBF16 ? 0x1p-7 + 0x1p-14 : (fmt == kFmtF16 ? 0x1p-10 + 0x1p-20 : 0.0);
  const double mf = fmt == kFmtBF16 ? 0x1p-8 + 0x1p-16 : (fmt == kFmtF16 ? 0x1p-11 + 0x1p-22 : 0.0);
  k += kf;
  SpecBracket o{0.f, 0.f, 0.f, 0.f, 1u, {0u, 0u, 0u}};  // deferred: c = 0 decides every level as 0
  if (ss > 0.0 && ss < 1e300 && k < 0.5) {
    const float n_lo = nextafterf((float)sqrt(ss * (1.0 - k)), 0.0f);
    const float n_hi = nextafterf((float)sqrt(ss * (1.0 + k)), INFINITY);
    if (n_lo >= 0x1p-90f && n_hi < INFINITY) {  // c_hi finite for L <= 2^30
      const double L = (double)a.e.levels;
      o.n_lo = n_lo;
      o.n_hi = n_hi;
      o.c_lo = nextafterf((float)(L / (double)n_hi * (1.0 - 0x1p-20) * (1.0 - mf)), 0.0f);
      o.c_hi = nextafterf((float)(L / (double)n_lo * (1.0 + 0x1p-20) * (1.0 + mf)), INFINITY);
      o.mode = 0u;
    }
  }
  return o;
}

template <bool WIDE, bool AQ>
__global__ __launch_bounds__(kBrThreads) void qsgd_spec_bracket(SpecArgs a, const SpecBrItem* __restrict__ items) {
  __shared__ double red[kBrWaves];
  __shared__ uint32_t s_last;
  spec_bracket_body<WIDE, AQ>(a, items, red, s_last);
}
// wide levels: two 1024-thread workgroups per CU (<= 64 VGPRs), so the kBrParts workgroups per
// tensor run in one generation
__global__ __launch_bounds__(kBrThreads) __attribute__((amdgpu_waves_per_eu(8))) void qsgd_spec_bracket_wide(
    SpecArgs a, const SpecBrItem* __restrict__ items) {
  __shared__ double red[kBrWaves];
  __shared__ uint32_t s_last;
  spec_bracket_body<true, false>(a, items, red, s_last);
}

// Levels of a quad for every norm of the bracket; und: some element is undecided.  u == 0 is
// raised to 2^-26 in the lower product only (x / n may underflow to 0 where |x| c does not:
// such an element is left undecided); a decided level needs no clamp (ceil(dl) <= the exact
// level <= L); NaN gives kl != kh.  scripts/exp/spec_check.c checks this exact form.
// und collects the wave's lane mask of undecided quads: each compare writes its mask to scalar
// registers and the four are or-ed there (a per-lane flag costs a select and a second compare to
// turn into the mask); a caller that has dead lanes masks them out.
__device__ __forceinline__ float raise_u(float u) {  // max(u, 2^-26) of a draw (>= +0, never NaN): an integer maximum
  return __uint_as_float(max(__float_as_uint(u), 0x32800000u));
}
__device__ __forceinline__ void spec_quad(float4 x, float4 u, float c_lo, float c_hi, int32_t (&q)[4], uint64_t& und) {
  const float xs[4] = {x.x, x.y, x.z, x.w}, us[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float ax = fabsf(xs[c]);
    const float kl = ceilf(fmaf(ax, c_lo, -raise_u(us[c])));
    const float kh = ceilf(fmaf(ax, c_hi, -us[c]));
    und |= __builtin_amdgcn_fcmpf(kl, kh, 14 /* une: kl != kh */);
    q[c] = (int32_t)copysignf(kh, xs[c]);
  }
}

// The same for bf16 / fp16 values (vn = x / n rounded to the format, a = |vn| L): the bracket's
// multipliers carry the format's relative rounding bound (qsgd_spec_bracket), and fp16's
// subnormal quotients (|vn| < 2^-14: an absolute step of 2^-24, i.e. at most 2^-25 L on a) take
// an absolute slack `dl` on both sides (u + dl is exact: u is a multiple of 2^-24 below 1).
// Every level between the two bounds' is then the level for some norm of the bracket, so
// kl == kh decides it; bf16 subnormals (|vn| < 2^-126) fall under the u == 0
// rule as in fp32.
__device__ __forceinline__ void spec_quad_fmt(float4 x, float4 u, float c_lo, float c_hi, float dl, int32_t (&q)[4],
                                              uint64_t& und) {
  const float xs[4] = {x.x, x.y, x.z, x.w}, us[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float ax = fabsf(xs[c]);
    const float kl = ceilf(fmaf(ax, c_lo, -(raise_u(us[c]) + dl)));
    const float kh = ceilf(fmaf(ax, c_hi, dl - us[c]));
    und |= __builtin_amdgcn_fcmpf(kl, kh, 14 /* une */);
    q[c] = (int32_t)copysignf(kh, xs[c]);
  }
}


// One block's pass: loads issued first, the Philox draws (independent of x) computed while
// they are in flight, then the partial, the levels and the undecided list.  FULL: a whole
// 4 Ki block (straight-line code, no bounds checks).
template <int WIDTH, bool FULL, bool DIV, uint32_t FMT, int AW = 0, int PW = kSpecPerWave, class GetBr>
__device__ __forceinline__ void spec_block(const SpecArgs& a, int64_t blk, int64_t b, int64_t end, int32_t t,
                                           int64_t tb, GetBr get_br, uint32_t* slot, uint64_t* part, float anorm,
                                           int tid) {
  const EncArgs& e = a.e;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: list and record bases are scalar
  float4 v[kSpecV];
  load_f4<kSpecV, FULL, true>(e.x, b, end, v, tid);  // x is read once: nontemporal (the fix uses the records)
  int4 araw[AW ? kSpecV : 1];
  if (AW) {  // the fused PS step's last client: its payload loaded beside x
#pragma unroll
    for (int k = 0; k < kSpecV; ++k)
      araw[k] = acc_load<AW ? AW : 1, FULL>(a.aq, b + 4 * ((int64_t)k * kThreads + tid), end);
  }
  float4 uu[4];
  philox_rows(e, b, tb, t, 0, uu, tid);
  // Branch-free from the loads to the stores, so that the scheduler can place the Philox
  // arithmetic under the load latency: x * alpha unconditionally (x * 1 = x; fp32 only, the
  // product is not rounded further), and levels computed for a deferred tensor too (its
  // multipliers are 0: every level 0, none undecided; the fix pass requantises it).
  const float alpha = e.alpha;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < kSpecV; ++k) {
    v[k] = mul4(v[k], alpha);
    if (FMT != kFmtF32 && alpha != 1.0f) v[k] = round_fmt4(v[k], FMT);  // torch.mul on the half tensor
    if (AW) {  // acc + decode(last client), stored when the caller keeps the accumulator
      v[k] = acc_add4<AW ? AW : 1>(v[k], araw[k], anorm, a.alevels, a.ainv);
      if (a.aout) {
        const int64_t el = b + 4 * ((int64_t)k * kThreads + tid);
        if (FULL || el + 4 <= end) {
          store_nt(a.aout + el, v[k]);
        } else if (el < end) {
          a.aout[el] = v[k].x;
          if (el + 1 < end) a.aout[el + 1] = v[k].y;
          if (el + 2 < end) a.aout[el + 2] = v[k].z;
        }
      }
    }
    if (DIV) {  // fused PS step: the average, stored once (nontemporal) and quantised from registers
      const float d = a.divisor;
      v[k].x = __fdiv_rn(v[k].x, d); v[k].y = __fdiv_rn(v[k].y, d);
      v[k].z = __fdiv_rn(v[k].z, d); v[k].w = __fdiv_rn(v[k].w, d);
      const int64_t el = b + 4 * ((int64_t)k * kThreads + tid);
      if (FULL || el + 4 <= end) {
        store_nt(a.xout + el, v[k]);
      } else if (el < end) {
        a.xout[el] = v[k].x;
        if (el + 1 < end) a.xout[el + 1] = v[k].y;
        if (el + 2 < end) a.xout[el + 2] = v[k].z;
      }
    }
    acc = sq4(v[k], acc);
  }
  const SpecBracket br = get_br();  // (the fused-bracket pass polls for it here, its loads in flight)
  uint32_t cnt = 0;  // wave-uniform
  {
    uint32_t* list = slot + PW * wave;
#pragma unroll
    for (int k = 0; k < kSpecV; ++k) {
      const int64_t el = b + 4 * ((int64_t)k * kThreads + tid);
      const bool live = FULL || el < end;
      int32_t qq[4];
      uint64_t m = 0;  // the wave's undecided quads
      if (FMT == kFmtF32) spec_quad(v[k], uu[k], br.c_lo, br.c_hi, qq, m);
      else spec_quad_fmt(v[k], uu[k], br.c_lo, br.c_hi, FMT == kFmtF16 ? 0x1p-25f * e.levels : 0.0f, qq, m);
      if (live) store_quad<WIDTH, FULL>(e, el, end, qq);
      if (!FULL) m &= __builtin_amdgcn_ballot_w64(live);
      if (m) {  // rare: list them
        const bool und = (m >> lane) & 1ull;
        const uint32_t pos =  // the listed quads of lower lanes (v_mbcnt: no lane mask built on the hot path)
            cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (live && und && pos < (uint32_t)PW) {  // the quad, its x and its draws: no re-read
          list[pos] = (uint32_t)(el >> 2);
          float4* rec = a.recs + 2 * ((blk * kWaves + wave) * PW + pos);
          rec[0] = v[k];
          rec[1] = uu[k];
        }
        cnt += (uint32_t)__popcll(m);
      }
    }
  }
  const double s = wave_sum_f64((double)acc);
  if (lane == 0) {
    *part = (uint64_t)__double_as_longlong(s);
    a.heads[blk * kWaves + wave] = ((uint32_t)t << 8) | min(cnt, (uint32_t)PW);
    if (cnt > (uint32_t)PW)
      __hip_atomic_fetch_or(&a.flags[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The per-tensor tables are __restrict__ const kernel arguments so that they are read with
// scalar loads (a vector load there is waited for before the x loads are issued).
// WPB: waves per workgroup.  A 4 Ki-element block's waves keep their element map (thread t of the
// block owns rows b + 4 (k 256 + t)), partials, heads and lists whatever the workgroup size; wide
// levels run one wave per workgroup (the int32 pass's shape: 0.508 against 0.534 ms for four waves,
// DESIGN.md §3.8).
template <int WIDTH, bool DIV, uint32_t FMT = kFmtF32, int AW = 0, int PW = kSpecPerWave, int WPB = kWaves>
__global__ __launch_bounds__(64 * WPB) void qsgd_spec_quant(SpecArgs a, const SpecBracket* __restrict__ brs,
                                                            const int64_t* __restrict__ begins,
                                                            const float* __restrict__ anorms) {
  static_assert(kWaves % WPB == 0, "a block's waves split evenly");
  constexpr int kPer = kWaves / WPB;  // workgroups per 4 Ki block
  const int64_t blk = blockIdx.x / kPer;
  const int tid = (int)(blockIdx.x % kPer) * 64 * WPB + (int)threadIdx.x;
  const Item it = a.e.items[blk >> 2];
  const SpecBracket br = brs[it.tensor];
  const int64_t tb = begins[it.tensor];
  const float anorm = AW ? anorms[it.tensor] : 0.0f;
  const int64_t b = it.begin + (blk & 3) * kSpecBlk;
  const int wave = tid >> 6;
  uint32_t* slot = a.slots + blk * spec_slot_words(PW);
  uint64_t* part = a.partials + blk * kWaves + wave;
  if (b >= it.end) {  // past the tensor's end: an empty block still reports (stale values otherwise)
    if ((tid & 63) == 0) {
      *part = 0ull;
      a.heads[blk * kWaves + wave] = (uint32_t)it.tensor << 8;
    }
    return;
  }
  const int64_t end = min(b + kSpecBlk, it.end);
  auto get_br = [&]() { return br; };
  if (end - b == kSpecBlk)
    spec_block<WIDTH, true, DIV, FMT, AW, PW>(a, blk, b, end, it.tensor, tb, get_br, slot, part, anorm, tid);
  else
    spec_block<WIDTH, false, DIV, FMT, AW, PW>(a, blk, b, end, it.tensor, tb, get_br, slot, part, anorm, tid);
}

// Fused bracket (OMF_SPEC_FB / omf_plan_set_fused_bracket): the bracket launch folded into the pass.
// Its first kFbParts x (bracket items) workgroups sample the tensors (256 threads each, an eighth of
// a tensor's runs; the last part to arrive combines the sums and publishes the multipliers as two
// {epoch, value} granules); the rest are the pass's blocks, which issue their loads and draws and
// then poll their tensor's granules.  The bracket workgroups have the lowest ids, so they are
// dispatched before any pass block and never wait; a pass block's poll is bounded anyway (20 ms and a
// minimum of polls): on expiry the tensor is flagged and requantised whole by the finish — exact.
// (kFbParts = 8 parts of 64 runs each: four float4 per thread, the pass's blocks' register budget)
//
// Wide levels (bit widths 5-8): the bracket folded into the one-wave pass the same way.  Its first
// kWfbParts x (bracket items) one-wave workgroups sample the tensors — part g of a tensor its runs
// g kPassesW .., every kWfbParts kPassesW-th round, kPassesW 1 KiB runs in flight per lane — and
// the last part of each tensor to arrive combines the 16 parts' sums in part order and publishes
// the multipliers; the pass's one-wave blocks poll them as qsgd_spec_quant_fb's do.  A bracket from
// other partial sums than the separate launch's may list other quads: the payload is exact either
// way (test_fused_bracket_equals_bracket_launch).
#ifndef OMF_WFB_PASSES  // experiment builds may override it (and kWfbParts, omf_plan_layout.h)
#define OMF_WFB_PASSES 8
#endif
constexpr int kPassesW = OMF_WFB_PASSES;

// A small tensor (n <= kSpecExact elements at x) read whole by NT threads, with its partial last quad:
// rounds of four float4 per thread, a round's fp32 chain added in fp64.
template <int NT>
__device__ __forceinline__ double whole_sumsq(const SpecArgs& a, const float* __restrict__ x, int64_t n) {
  double s = 0.0;
  for (int64_t r0 = 0; r0 < n; r0 += 16 * NT) {
    float4 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t e = r0 + 4 * ((int64_t)i * NT + threadIdx.x);
        v[i] = e + 4 <= n ? *reinterpret_cast<const float4*>(x + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < n && e + 4 > n) {  // the tensor's partial last quad
          v[i].x = x[e];
          if (e + 1 < n) v[i].y = x[e + 1];
          if (e + 2 < n) v[i].z = x[e + 2];
        }
      }
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = sq4(spec_prologue(v[i], a.e.alpha, a.divisor, a.e.fmt), acc);
    s += (double)acc;
  }
  return s;
}

// Workgroup wg of a fused pass launch: part wg % PARTS of the bracket of tensor wg / PARTS, NT threads
// (one wave, summed by its butterfly, or kThreads, summed by block_sum_f64) sampling runs of RUN
// elements, PASSES of them in flight per lane.  The last part of a tensor to arrive writes its
// bracket and publishes the multipliers.
template <int NT, int PARTS, int RUN, int PASSES>
__device__ __forceinline__ void spec_bracket_part(const SpecArgs& a, const SpecBrItem* __restrict__ items, int64_t wg) {
  static_assert(NT == 64 || NT == kThreads, "one wave, or block_sum_f64's workgroup");
  const int part = (int)(wg % PARTS);
  const SpecBrItem bi = items[wg / PARTS];
  const int32_t t = bi.tensor;
  const int64_t tb = bi.begin, n = bi.n, R = RUN == kSpecRunWide ? bi.Rw : bi.R;
  const float* __restrict__ x = a.e.x + tb;
  const bool exact = n <= kSpecExact;
  if (exact && part != 0) return;
  double s1 = 0.0, s2 = 0.0;
  if (exact) s1 = whole_sumsq<NT>(a, x, n);
  else bracket_sample<RUN, false, NT, PASSES>(a, x, t, tb, n, R, part, PARTS, s1, s2);
  double S[2];
  if constexpr (NT == 64) {
    S[0] = wave_sum_f64(s1);
    S[1] = wave_sum_f64(s2);
    if (threadIdx.x != 0) return;
  } else {
    __shared__ double red[kWaves];
    S[0] = block_sum_f64(s1, red);
    S[1] = block_sum_f64(s2, red);
  }
  if (!exact) {  // the last part to arrive combines the partials in part order
    uint64_t* bp = reinterpret_cast<uint64_t*>(a.br_part);
    bool last;
    if constexpr (NT == 64) {
      last = arrive_last(bp, t, part, S, a.br_cnt, t, PARTS);
    } else {
      __shared__ uint32_t s_last;
      last = arrive_last_block(bp, t, part, S, a.br_cnt, t, PARTS, s_last);
    }
    if (!last) return;
    combine_parts(bp, t, PARTS, S);
  }
  if (threadIdx.x != 0) return;
  const SpecBracket o = bracket_from_sums(a, exact, n, R, RUN, S[0], S[1]);
  a.br[t] = o;  // the finish launch reads it (a later launch)
  const uint64_t ep = (uint64_t)a.epoch << 32;
  st_agent(&a.brgran[2 * t], ep | __float_as_uint(o.c_lo));
  st_agent(&a.brgran[2 * t + 1], ep | __float_as_uint(o.c_hi));
}

// The pass blocks' poll for their tensor's fused bracket (bounded: on expiry the tensor is flagged
// and requantised whole by the finish — exact; the sampling workgroups have the lowest ids, so they
// are dispatched before any pass block and never wait).
__device__ __forceinline__ SpecBracket fb_poll(const SpecArgs& a, int32_t t) {
  uint64_t g0 = ld_agent(&a.brgran[2 * t]), g1 = ld_agent(&a.brgran[2 * t + 1]);
  if ((uint32_t)(g0 >> 32) != a.epoch || (uint32_t)(g1 >> 32) != a.epoch) {
    const uint64_t t0 = wall_clock64(), min_polls = a.wait_ticks >> 10;
    uint64_t polls = 0;
    for (int k = 0;; k = min(k + 1, 6)) {
      if (k < 2) __builtin_amdgcn_s_sleep(2);
      else __builtin_amdgcn_s_sleep(8);
      g0 = ld_agent(&a.brgran[2 * t]);
      g1 = ld_agent(&a.brgran[2 * t + 1]);
      if ((uint32_t)(g0 >> 32) == a.epoch && (uint32_t)(g1 >> 32) == a.epoch) break;
      if (++polls > min_polls && wall_clock64() - t0 > a.wait_ticks) {  // never expected: requantise whole
        __hip_atomic_fetch_or(&a.flags[t], 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g0 = g1 = 0;
        break;
      }
    }
  }
  return SpecBracket{__uint_as_float((uint32_t)g0), __uint_as_float((uint32_t)g1), 0.f, 0.f, 0u, {0u, 0u, 0u}};
}

// A fused pass's block, one copy for qsgd_spec_quant_fb and _wfb: thread tid (0 .. 255) of the 4 Ki block
// blk — its item, range, list slot and wave's partial, then the block's pass (whole or not), which polls
// for the tensor's bracket.  An empty block (past the tensor's end) still reports its partial and head
// (stale values otherwise).  qsgd_spec_quant keeps the same header in its own body: going through this
// function, its int8 kernels came out with the two operands of one v_or_b32 exchanged.
template <int WIDTH, bool DIV, int PW>
__device__ __forceinline__ void fused_pass_block(const SpecArgs& a, int64_t blk, int tid,
                                                 const int64_t* __restrict__ begins) {
  const Item it = a.e.items[blk >> 2];
  const int32_t t = it.tensor;
  const int64_t tb = begins[t];
  const int64_t b = it.begin + (blk & 3) * kSpecBlk;
  const int wave = tid >> 6;
  uint32_t* slot = a.slots + blk * spec_slot_words(PW);
  uint64_t* part = a.partials + blk * kWaves + wave;
  if (b >= it.end) {
    if ((tid & 63) == 0) {
      *part = 0ull;
      a.heads[blk * kWaves + wave] = (uint32_t)t << 8;
    }
    return;
  }
  auto get_br = [&]() { return fb_poll(a, t); };
  const int64_t end = min(b + kSpecBlk, it.end);
  if (end - b == kSpecBlk)
    spec_block<WIDTH, true, DIV, kFmtF32, 0, PW>(a, blk, b, end, t, tb, get_br, slot, part, 0.0f, tid);
  else
    spec_block<WIDTH, false, DIV, kFmtF32, 0, PW>(a, blk, b, end, t, tb, get_br, slot, part, 0.0f, tid);
}

template <int WIDTH, bool DIV>
__global__ __launch_bounds__(kThreads) void qsgd_spec_quant_fb(SpecArgs a, const SpecBrItem* __restrict__ bitems,
                                                               int64_t nbrw, const int64_t* __restrict__ begins) {
  if ((int64_t)blockIdx.x < nbrw) {
    spec_bracket_part<kThreads, kFbParts, kSpecRun, 4>(a, bitems, blockIdx.x);
    return;
  }
  fused_pass_block<WIDTH, DIV, kSpecPerWave>(a, (int64_t)blockIdx.x - nbrw, (int)threadIdx.x, begins);
}

template <int WIDTH, bool DIV>
__global__ __launch_bounds__(64) void qsgd_spec_quant_wfb(SpecArgs a, const SpecBrItem* __restrict__ bitems,
                                                          int64_t nbrw, const int64_t* __restrict__ begins) {
  if ((int64_t)blockIdx.x < nbrw) {
    spec_bracket_part<64, kWfbParts, kSpecRunWide, kPassesW>(a, bitems, blockIdx.x);
    return;
  }
  const int64_t wgi = (int64_t)blockIdx.x - nbrw;
  fused_pass_block<WIDTH, DIV, kSpecPerWaveWide>(a, wgi / kWaves, (int)(wgi % kWaves) * 64 + (int)threadIdx.x, begins);
}

// One fold segment (a workgroup of the finish launch); the last arriver of the tensor folds the
// segments in order, checks the bracket and publishes {epoch, bad, norm} in the tensor's granule.
__device__ void spec_fold(const SpecArgs& a, const SpecFoldItem& fi) {
  __shared__ double red[kWaves];
  __shared__ uint32_t s_last;
  const int32_t t = fi.tensor;
  // up to kSpecSeg partials: 16 loads in flight per thread, a fixed order
  constexpr int U = kSpecSeg / kThreads;
  double v[U];
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const int64_t j = fi.p_begin + threadIdx.x + (int64_t)i * kThreads;
    const double d = __longlong_as_double((long long)a.partials[j < fi.p_end ? j : fi.p_begin]);  // unconditional load
    v[i] = j < fi.p_end ? d : 0.0;
  }
  double p = 0.0;
#pragma unroll
  for (int i = 0; i < U; ++i) p += v[i];
  double tot = block_sum_f64(p, red);
  if (fi.nsegs > 1) {
    const double seg[1] = {tot};
    if (!arrive_last_block(a.seg_part, 0, fi.sbase + fi.seg, seg, a.fold_cnt, t, fi.nsegs, s_last)) return;
    double q = 0.0;
    for (int j = threadIdx.x; j < fi.nsegs; j += kThreads)
      q += __longlong_as_double((long long)ld_agent(&a.seg_part[fi.sbase + j]));
    tot = block_sum_f64(q, red);
  }
  if (threadIdx.x != 0) return;
  const float norm = finish_norm(tot, a.e.fmt);
  a.e.norm_out[t] = norm;
  const SpecBracket br = a.br[t];
  const uint32_t fl = a.flags[t];
  const bool ok = br.mode == 0u && fl == 0u && norm >= br.n_lo && norm <= br.n_hi;
  a.status[t] = ok ? 0u : 1u;
  if (fl) a.flags[t] = 0u;
  st_agent(&a.ngran[t], ((uint64_t)((a.epoch << 1) | (ok ? 0u : 1u)) << 32) | __float_as_uint(norm));
}

// The tensor's norm and status as its fold published them in this launch (bounded; the fold
// workgroups are dispatched before every fix workgroup and never wait, so the bound is only a
// guard against a logic error).  false: timed out (err bit 4 set, reported as OMF_ETIMEOUT by
// omf_plan_check, which every product entry point calls).  The bound needs the wall-clock
// time AND a minimum number of polls, so a context switch of the queue (the clock runs on
// while the wave is saved) cannot fake an expiry.
__device__ __forceinline__ bool spec_norm_wait(const SpecArgs& a, int32_t t, float& norm, bool& bad) {
  uint64_t g = ld_agent(&a.ngran[t]);
  if ((uint32_t)(g >> 33) != a.epoch) {
    // exponential back-off: every polling wave reads one of 183-odd granules, and tight
    // polling of a few lines by tens of thousands of waves congests them
    const uint64_t t0 = wall_clock64();
    const uint64_t min_polls = a.wait_ticks >> 10;  // a back-off poll is <= ~200 ticks
    uint64_t polls = 0;
    for (int k = 0;; k = min(k + 1, 6)) {
      if (k < 2) __builtin_amdgcn_s_sleep(4);
      else if (k < 4) __builtin_amdgcn_s_sleep(16);
      else __builtin_amdgcn_s_sleep(64);
      g = ld_agent(&a.ngran[t]);
      if ((uint32_t)(g >> 33) == a.epoch) break;
      if (++polls > min_polls && wall_clock64() - t0 > a.wait_ticks) {
        __hip_atomic_fetch_or(a.e.err, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return false;
      }
    }
  }
  norm = __uint_as_float((uint32_t)g);
  bad = ((g >> 32) & 1u) != 0u;
  return true;
}

// The finish launch: its first nfold workgroups fold the partials (spec_fold); the rest fix the
// listed quads, one thread per wave slot: (the slot header), then (the block's item) with the
// tensor's norm granule, then per listed quad its index, recorded x and draws, the exact level
// from the shared element math (Markstein division) and its store.  A block whose tensor the fold marked bad (norm outside the bracket, a slot
// overflow, a deferred tensor) is requantised whole from x by its workgroup (the rare path).
template <int WIDTH, int PW = kSpecPerWave, int FT = 1>
__global__ __launch_bounds__(kThreads) void qsgd_spec_finish(SpecArgs a, const SpecFoldItem* __restrict__ fold_items,
                                                             int32_t nfold, const Item* __restrict__ items,
                                                             const int64_t* __restrict__ begins,
                                                             const uint32_t* __restrict__ slots,
                                                             const float4* __restrict__ recs,
                                                             const uint32_t* __restrict__ heads) {
  if ((int32_t)blockIdx.x < nfold) {
    if (!(a.dbg & 16u)) spec_fold(a, fold_items[blockIdx.x]);  // test hook: no fold, the fix waits expire
    return;
  }
  // FT threads per wave slot (its listed quads in turn, strided: narrow levels list none or one, so
  // FT = 1 there — 8 threads per slot took 8x the workgroups: +8-10 us; wide levels list ~10 per
  // slot, FT = 4), kThreads / (kWaves FT) blocks per workgroup: the fix is a few dependent round
  // trips per thread, so its cost is the number of workgroup generations, not the quads.
  constexpr int BPW = kThreads / (kWaves * FT);  // blocks per workgroup
  __shared__ uint32_t s_rep[BPW];
  __shared__ float s_rep_norm[BPW];  // the granule's norm (norm_out is written in this launch)
  __shared__ uint32_t s_nrep;
  const EncArgs& e = a.e;
  const int64_t fb = (int64_t)blockIdx.x - nfold;
  if (threadIdx.x == 0) s_nrep = 0u;
  const int64_t ws = (fb * kThreads + threadIdx.x) / FT;  // global wave slot
  const uint32_t sub = (uint32_t)(threadIdx.x % FT);
  const int64_t blk = ws / kWaves;
  const int w = (int)(ws % kWaves);
  bool rep = false;
  float rep_norm = 0.0f;
  if (blk < a.nblocks) {
    const uint32_t head = heads[ws];
    const uint32_t cnt = head & 0xffu;
    const int32_t t = (int32_t)(head >> 8);
    const bool leader = w == 0 && sub == 0;  // one status check per block
    if ((cnt > 0u || leader) && !(a.dbg & 8u)) {
      // this thread's first PRE listed quads (index, recorded x and draws) are loaded before the
      // norm wait, so their round trip overlaps it (clamped to the last listed quad: no load
      // under a branch); the rest, if any (narrow lists only), in the loop after
      constexpr int PRE = FT > 1 ? PW / FT : 0;  // (narrow lists: usually empty, the loop below)
      uint32_t qv[PRE > 0 ? PRE : 1];
      float4 rx[PRE > 0 ? PRE : 1], ru[PRE > 0 ? PRE : 1];
      const uint32_t jl = cnt > 0u ? cnt - 1u : 0u;
#pragma unroll
      for (int k = 0; k < PRE; ++k) {
        const uint32_t j = min(sub + (uint32_t)(k * FT), jl);
        qv[k] = slots[blk * spec_slot_words(PW) + PW * w + j];
        rx[k] = recs[2 * (ws * PW + j)];
        ru[k] = recs[2 * (ws * PW + j) + 1];
      }
      const Item it = items[blk >> 2];
      float norm;
      bool bad;
      if (spec_norm_wait(a, t, norm, bad)) {
        const int64_t b = it.begin + (blk & 3) * kSpecBlk, end = min(b + kSpecBlk, it.end);
        const Divisor dv(norm, e.fmt);
#pragma unroll
        for (int k = 0; k < PRE; ++k) {
          if (sub + (uint32_t)(k * FT) >= cnt) break;
          int32_t qq[4];
          qsgd_quad<false>(rx[k], ru[k], dv, e.levels, false, qq);
          if (!(a.dbg & 4u)) store_quad<WIDTH>(e, 4 * (int64_t)qv[k], end, qq);
        }
        for (uint32_t j = sub + (uint32_t)(PRE * FT); j < cnt; j += FT) {
          const uint32_t q = slots[blk * spec_slot_words(PW) + PW * w + j];
          const float4* rec = recs + 2 * (ws * PW + j);
          int32_t qq[4];
          qsgd_quad<false>(rec[0], rec[1], dv, e.levels, false, qq);
          if (!(a.dbg & 4u)) store_quad<WIDTH>(e, 4 * (int64_t)q, end, qq);
        }
        rep = leader && bad;
        rep_norm = norm;
      }
    }
  }
  __syncthreads();  // s_nrep initialised
  if (rep) {
    const uint32_t i = atomicAdd(&s_nrep, 1u);
    s_rep[i] = (uint32_t)(blk - fb * BPW);
    s_rep_norm[i] = rep_norm;
  }
  if (!__syncthreads_or(rep)) return;
  const uint32_t nrep = s_nrep;
  EncArgs er = e;  // the fused PS step requantises from the average the pass wrote
  if (a.divisor != 0.0f) {
    er.x = a.xout;
    er.alpha = 1.0f;
  }
  for (uint32_t r = 0; r < nrep; ++r) {  // whole blocks of requantised tensors, all 256 threads
    const int64_t rb = fb * BPW + s_rep[r];
    const Item it = items[rb >> 2];
    const int64_t b = it.begin + (rb & 3) * kSpecBlk;
    if (b < it.end)
      quant_sub<WIDTH, false, kSpecV>(er, b, min(b + kSpecBlk, it.end), begins[it.tensor], it.tensor, s_rep_norm[r]);
  }
}

}  // namespace

// The buffers of the wide levels (bit widths 5-8), made at a plan's first wide encode: slots and
// records of the wide list capacity, the bracket parts' partial sums and arrival counters.
static int ensure_wide(omf_plan* p, hipStream_t st) {
  if (p->d_spec_slots_w) return OMF_OK;
  const size_t nt = (size_t)p->nt, nb = (size_t)p->n_spec_blocks;
  Carve c;
  c.raw(p->d_spec_slots_w, (size_t)spec_slot_words(kSpecPerWaveWide) * nb);
  c.raw(p->d_spec_recs_w, 2 * (size_t)kWaves * kSpecPerWaveWide * nb);
  c.raw(p->d_spec_br_part, 2 * (size_t)kBrParts * nt);
  c.zero(p->d_spec_br_cnt, nt);  // left zero by every launch
  return make_buffers(p, c, st);
}

// The fused bracket's, made at the first encode that folds the bracket into the pass: its parts'
// partial sums, arrival counters and granules.
static int ensure_fused_bracket(omf_plan* p, hipStream_t st) {
  if (p->d_spec_fb_part) return OMF_OK;
  const size_t nt = (size_t)p->nt;
  Carve c;
  c.raw(p->d_spec_fb_part, 2 * (size_t)std::max(kFbParts, kWfbParts) * nt);
  c.zero(p->d_spec_fb_cnt, nt);      // left zero by every launch
  c.zero(p->d_spec_brgran, 2 * nt);  // epoch 0 is never a launch's tag
  return make_buffers(p, c, st);
}

// Bracketed single-read encoder: the bracket (a launch of its own, or the first workgroups of the
// pass), the pass, the finish.  No host interaction.  Each kernel comes from a table indexed by
// the variant (wide levels, fused bracket), the payload width, the fused PS step's divide, the
// value format and the fused last client's payload width.
int omf::bracket::launch(omf_plan* p, const EncCall& c, const Choice& ch) {
  using BracketKernel = void (*)(SpecArgs, const SpecBrItem*);
  using PassKernel = void (*)(SpecArgs, const SpecBracket*, const int64_t*, const float*);
  using FusedKernel = void (*)(SpecArgs, const SpecBrItem*, int64_t, const int64_t*);
  using FinishKernel = void (*)(SpecArgs, const SpecFoldItem*, int32_t, const Item*, const int64_t*, const uint32_t*,
                                const float4*, const uint32_t*);
  constexpr int PWW = kSpecPerWaveWide;
#ifndef OMF_FIX_FT  // experiment builds may override it (profiles/r05_s8_variants.txt)
#define OMF_FIX_FT 4
#endif
  constexpr int FT = OMF_FIX_FT;  // the wide finish: fix threads per wave slot
  static const BracketKernel k_bracket[2] = {qsgd_spec_bracket<false, false>, qsgd_spec_bracket<false, true>};  // [last client]
  static const FusedKernel k_fb[2] = {qsgd_spec_quant_fb<1, false>, qsgd_spec_quant_fb<1, true>};  // [divide]
  static const FusedKernel k_wfb[2][2] = {{qsgd_spec_quant_wfb<1, false>, qsgd_spec_quant_wfb<1, true>},  // [int32 wire][divide]
                                          {qsgd_spec_quant_wfb<4, false>, qsgd_spec_quant_wfb<4, true>}};
  static const PassKernel k_pass[2][2] = {{qsgd_spec_quant<1, false>, qsgd_spec_quant<1, true>},  // [int32 wire][divide]
                                          {qsgd_spec_quant<4, false>, qsgd_spec_quant<4, true>}};
  static const PassKernel k_pass_half[2] = {qsgd_spec_quant<1, false, kFmtBF16>, qsgd_spec_quant<1, false, kFmtF16>};
  static const PassKernel k_pass_last[2] = {qsgd_spec_quant<1, true, kFmtF32, 1>,  // [the last client's int32 payload]
                                            qsgd_spec_quant<1, true, kFmtF32, 4>};
  static const PassKernel k_pass_wide[2][2][2] = {  // [four waves per workgroup][int32 wire][divide]
      {{qsgd_spec_quant<1, false, kFmtF32, 0, PWW, 1>, qsgd_spec_quant<1, true, kFmtF32, 0, PWW, 1>},
       {qsgd_spec_quant<4, false, kFmtF32, 0, PWW, 1>, qsgd_spec_quant<4, true, kFmtF32, 0, PWW, 1>}},
      {{qsgd_spec_quant<1, false, kFmtF32, 0, PWW>, qsgd_spec_quant<1, true, kFmtF32, 0, PWW>},
       {qsgd_spec_quant<4, false, kFmtF32, 0, PWW>, qsgd_spec_quant<4, true, kFmtF32, 0, PWW>}}};
  static const FinishKernel k_finish[2][2] = {{qsgd_spec_finish<1>, qsgd_spec_finish<4>},  // [wide][int32 wire]
                                              {qsgd_spec_finish<1, PWW, FT>, qsgd_spec_finish<4, PWW, FT>}};
  // The wide pass's one-wave workgroups reserve 10 KiB of LDS each (unused): 16 per CU, i.e. four
  // waves per SIMD — 0.556-0.559 ms per Llama-400M s = 8 encode against 0.589 uncapped, 0.565 at 12
  // KiB, 0.635 at 16 KiB (two interleaved rounds); OMF_SPEC_LDS_W overrides.
  // The s <= 4 pass lost under a cap at first (24 KiB: 0.367 against 0.360 ms); since its wave sum left
  // the LDS and its quad math shed a tenth of its VALU work it reserves 24 KiB (unused): six workgroups
  // per CU, where the registers would admit eight (profiles/r07_pass_schedule_ab.txt;
  // OMF_SPEC_LDS overrides).  The fused PS step's pass, which also stores the average, is not capped (not
  // measured); nor is a pass without the fused bracket.  Wide unfused: one wave per workgroup unless
  // OMF_SPEC_WPB=4.
  static const size_t plds_w = [] { const char* v = omf::knob("OMF_SPEC_LDS_W"); return v ? (size_t)atoi(v) : (size_t)10240; }();
  static const size_t plds_n = [] { const char* v = omf::knob("OMF_SPEC_LDS"); return v ? (size_t)atoi(v) : (size_t)24576; }();
  static const bool wpb4 = [] { const char* v = omf::knob("OMF_SPEC_WPB"); return v && atoi(v) == 4; }();

  const hipStream_t st = c.st;
  const AccIn* acc = c.acc_in;
  const bool wide = ch.wide, div = c.divisor != 0.0f, w4 = c.width == 4;
  if (wide)
    if (int r = ensure_wide(p, st)) return r;
  if (ch.fused)
    if (int r = ensure_fused_bracket(p, st)) return r;
  SpecArgs sa;
  sa.e = enc_args(p, c);
  sa.e.items = p->d_flat;
  sa.e.tinfo = p->d_tinfo[1];
  sa.begins = p->d_begins;
  sa.sizes = p->d_sizes;
  sa.br_items = p->d_spec_br_items;
  sa.fold_items = p->d_spec_fold_items;
  sa.seg_part = p->d_spec_seg_part;
  sa.fold_cnt = p->d_spec_cnt;
  if (++p->spec_epoch >= 0x80000000u) p->spec_epoch = 1;  // 31-bit tags (the norm granule keeps a status bit)
  sa.epoch = p->spec_epoch;
  sa.wide = wide ? 1u : 0u;
  sa.ngran = p->d_spec_ngran;
  // p->spec_skip: test / experiment switches (omf_plan_set_debug; 0 in production): bit 0
  // skips the bracket launch (the previous brackets stay), bit 1 the finish launch, bits 2/3
  // the fix stores / the fix, bit 4 the fold — the payload is then not the encoder's.
  sa.dbg = p->spec_skip;
  sa.zsig = wide ? p->spec_zsig_wide : p->spec_zsig;
  sa.divisor = c.divisor;
  sa.xout = c.xout;
  sa.wait_ticks = p->wait_ticks;
  sa.br = p->d_spec_br;
  sa.partials = p->d_spec_part;
  sa.br_part = ch.fused ? p->d_spec_fb_part : p->d_spec_br_part;
  sa.br_cnt = ch.fused ? p->d_spec_fb_cnt : p->d_spec_br_cnt;
  sa.brgran = p->d_spec_brgran;
  p->spec_last_pw = wide ? kSpecPerWaveWide : kSpecPerWave;
  sa.slots = wide ? p->d_spec_slots_w : p->d_spec_slots;
  sa.heads = p->d_spec_heads;
  sa.recs = wide ? p->d_spec_recs_w : p->d_spec_recs;
  sa.flags = p->d_spec_flags;
  sa.status = p->d_spec_status;
  sa.nblocks = p->n_spec_blocks;
  sa.aq = acc ? acc->q : nullptr;
  sa.anorm = acc ? acc->norm : nullptr;
  sa.aout = acc ? acc->acc_out : nullptr;
  sa.awidth = acc ? acc->width : 0;
  sa.alevels = acc ? (float)acc->levels : 0.0f;
  sa.ainv = acc && (acc->levels & (acc->levels - 1)) == 0 ? 1.0f / (float)acc->levels : 0.0f;

  const int64_t nb = p->n_spec_blocks, nt = p->nt;
  if (ch.bracket_launch)
    launch_kernel(wide ? qsgd_spec_bracket_wide : k_bracket[acc != nullptr], dim3((unsigned)(nt * (wide ? kBrParts : 1))),
           dim3(kBrThreads), 0, st, sa, sa.br_items);
  if (ch.fused) {  // the bracket's parts are the pass launch's first workgroups; wide: one-wave workgroups
    const int64_t nbrw = (wide ? kWfbParts : kFbParts) * nt;
    if (wide) launch_kernel(k_wfb[w4][div], dim3((unsigned)(nbrw + nb * kWaves)), dim3(64), plds_w, st, sa, sa.br_items, nbrw, sa.begins);
    else launch_kernel(k_fb[div], dim3((unsigned)(nbrw + nb)), dim3(kThreads), div ? 0 : plds_n, st, sa, sa.br_items, nbrw, sa.begins);
  } else if (wide && !wpb4) {
    launch_kernel(k_pass_wide[0][w4][div], dim3((unsigned)(nb * kWaves)), dim3(64), plds_w, st, sa, sa.br, sa.begins, sa.anorm);
  } else {
    const PassKernel k = wide                 ? k_pass_wide[1][w4][div]
                         : c.fmt == kFmtBF16 ? k_pass_half[0]
                         : c.fmt == kFmtF16  ? k_pass_half[1]
                         : acc               ? k_pass_last[acc->width == 32]
                                             : k_pass[w4][div];
    launch_kernel(k, dim3((unsigned)nb), dim3(kThreads), 0, st, sa, sa.br, sa.begins, sa.anorm);
  }
  if (!(p->spec_skip & 2u)) {  // (experiment: no finish launch, timings only)
    // the fold's workgroups first, then the fix: a workgroup's threads share kWaves (x FT, wide) per block
    const int64_t per = kThreads / (kWaves * (wide ? FT : 1));
    const int32_t nfold = (int32_t)p->n_spec_fold;
    launch_kernel(k_finish[wide][w4], dim3((unsigned)(nfold + (nb + per - 1) / per)), dim3(kThreads), 0, st, sa, sa.fold_items,
           nfold, sa.e.items, sa.begins, sa.slots, sa.recs, sa.heads);
  }
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}
