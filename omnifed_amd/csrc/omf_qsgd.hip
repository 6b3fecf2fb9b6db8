// omf_qsgd.hip — the QSGD plan, encoders and PS steps for the hybrid global hop, MI355X (gfx950).
//
// Semantics: SURVEY.md §8a "Exact QSGD semantics", restating
//   src/omnifed/hybrid/compression/qsgd.py:36-96 (reference, Python/torch CPU).
//
// Kernel map (the bracketed single-read encoder, strategy 3, is omf_qsgd_bracket.hip
// and the single-read ring encoder omf_qsgd_ring.hip; the device steps the encoders share are
// omf_qsgd_enc.h; the decoders, the K-client sum and the flat divide are omf_qsgd_recv.hip).  Every
// encoder writes the same payload bits for the same norm.
//   qsgd_encode_ordered    ticket-ordered encoder (strategies 0 and 1, and every norms-only pass): one
//                          launch for every tensor.  Work items are taken in ticket order (an atomic
//                          counter, so a workgroup only waits on items that are already running):
//                          RESIDENT(t) holds its elements in registers, publishes the fp64 partial
//                          sum of squares, waits for the tensor norm and quantises — x read once;
//                          NORM(t) / QUANT(t) are the two passes of a larger tensor.  The last
//                          arriver of a tensor folds its partials in fixed order (deterministic norm)
//                          and publishes a {tag, norm} granule that the waiters poll.
//   qsgd_quant_sub         norms supplied by the caller: one pass over the flat items, no hand-off.
//   qsgd_encode_grid       grid encoder (strategy 4, small arenas): one workgroup per CU, x held in
//                          registers across one grid-wide barrier.
//   items_f32_kernel       dst = src / d or src over the tensors' elements only (the in-place PS step,
//                          the last client's two-call fallback): arena padding is never written.
//
// Host side (the end of the file): omf_plan_create / upload_plan carve the plan's device block from
// the tables of omf_plan_layout.cpp; encode_launch asks choose_encoder (omf_plan_layout.h) which
// encoder serves a call and switches over five launchers (caller norms, grid, bracket — omf_bracket.h —,
// ring — omf_ring.h —, ordered); the omf_ps_* steps are that switch and, where the bracketed encoder does not
// take the last client's payload itself, omf_qsgd_decode (omf_qsgd_recv.hip).  struct omf_plan is in omf_plan.h.
//
// HBM-bound; no MFMA (no contraction).  Coalesced 16 B/lane fp32 loads, non-temporal
// 16 B/lane fp32 and 4 B/lane int8 payload stores.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/omf_codec.h"
#include "../../include/omf_codec_experimental.h"
#include "omf_bracket.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_dec.h"
#include "omf_qsgd_enc.h"
#include "omf_ring.h"

using namespace omf;
using namespace omf::plan_layout;  // the table records and layout constants (omf_plan_layout.h)

namespace {

static_assert(kBlkWaves == kWaves, "one wave partial per wave of a block's workgroup");

// ---------------------------------------------------------------- norm hand-off

// Sum of squares of one item's range, exactly as a NORM item computes it: sub-chunks in
// order, each thread accumulating its own rows in fp32.
template <int V>
__device__ __forceinline__ float chunk_sumsq(const EncArgs& a, int64_t b, int64_t e) {
  constexpr int64_t S = (int64_t)V * 1024;
  float acc = 0.0f;
  for (int64_t sb = b; sb < e; sb += S) {
    const int64_t se = min(sb + S, e);
    float4 v[V];
    if (se - sb == S) load_f4<V, true>(a.x, sb, se, v);  // default policy: the QUANT re-read hits the Infinity Cache
    else load_f4<V, false>(a.x, sb, se, v);
    scale_f4<V>(v, a);
    acc = sumsq_f4<V>(v, acc);
  }
  return acc;
}

struct HandoffShared {
  double red[kWaves];
  uint32_t last, ok;
  float norm;
};

// Publish one item's partial; the last arriver of the tensor folds all partials in a fixed
// order (deterministic norm) and publishes the {tag = 1, norm} granule.  Protocol
// (cdna_hip_programming.md §6 G16): partial stored sc1 and drained before the
// agent-scope counter add; the last arriver reads the partials with sc1 loads.
__device__ __forceinline__ void publish_partial(const EncArgs& a, const TensorInfo& ti, int32_t t, int32_t idx,
                                                float acc, HandoffShared& sh) {
  const double s = block_sum_f64((double)acc, sh.red);
  if (threadIdx.x == 0) {
    st_agent(&a.partials[ti.pbase + idx], (uint64_t)__double_as_longlong(s));
    drain_vmem();
    const uint32_t old = add_agent(&a.counters[t], 1u);
    sh.last = (old == (uint32_t)(ti.nchunks - 1)) ? 1u : 0u;
    // Every partial of t has arrived: reset the counter for the next launch (stream order).
    if (sh.last) __hip_atomic_store(&a.counters[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (sh.last) {
    double p = 0.0;
    for (int j = threadIdx.x; j < ti.nchunks; j += kThreads)
      p += __longlong_as_double((long long)ld_agent(&a.partials[ti.pbase + j]));
    const double tot = block_sum_f64(p, sh.red);
    if (threadIdx.x == 0) {
      const float norm = finish_norm(tot, a.fmt);
      a.norm_out[t] = norm;
      st_agent(&a.gran[t], ((uint64_t)a.epoch << 32) | (uint64_t)__float_as_uint(norm));
    }
  }
}

// Poll the tensor's granule (one lane, relaxed sc1 loads, bounded).  On timeout (the
// tensor's items were not all co-resident) recompute every partial exactly as its owner
// does and fold them in the last arriver's order: identical bits, err bit 2 set.
template <int V>
__device__ __forceinline__ float norm_wait_or_recompute(const EncArgs& a, const TensorInfo& ti, int32_t t,
                                                        HandoffShared& sh) {
  if (threadIdx.x == 0) {
    const uint64_t t0 = wall_clock64();
    uint32_t ok = 0;
    float nv = 0.0f;
    for (;;) {
      const uint64_t g = ld_agent(&a.gran[t]);
      if ((uint32_t)(g >> 32) == a.epoch) {
        nv = __uint_as_float((uint32_t)g);
        ok = 1;
        break;
      }
      if (wall_clock64() - t0 > a.wait_ticks) break;
      __builtin_amdgcn_s_sleep(1);
    }
    sh.norm = nv;
    sh.ok = ok;
  }
  __syncthreads();
  const float nv = sh.norm;
  const uint32_t ok = sh.ok;
  __syncthreads();
  if (ok) return nv;
  double p = 0.0;
  for (int j = 0; j < ti.nchunks; ++j) {
    const int64_t b = ti.begin + (int64_t)j * ti.chunk, e = min(b + ti.chunk, ti.begin + ti.n);
    const double sj = block_sum_f64((double)chunk_sumsq<V>(a, b, e), sh.red);
    if ((j % kThreads) == (int)threadIdx.x) p += sj;
  }
  const double tot = block_sum_f64(p, sh.red);
  if (threadIdx.x == 0) __hip_atomic_fetch_or(a.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return finish_norm(tot, a.fmt);
}

// ---------------------------------------------------------------- kernels

// EV: float4 rows per thread of one encode sub-chunk (EV * 1024 elements); RESIDENT items
// are one sub-chunk, NORM/QUANT items loop over the sub-chunks of their chunk.
template <int WIDTH, bool HAS_U, bool NORM_ONLY, int EV>
__global__ __launch_bounds__(kThreads) void qsgd_encode_ordered(EncArgs a) {
  constexpr int64_t ES = (int64_t)EV * 1024;
  __shared__ HandoffShared sh;
  __shared__ uint32_t s_ticket;
  if (threadIdx.x == 0) {
    const uint32_t tk = add_agent(a.ticket, 1u);
    // The last ticket of the launch: every workgroup has taken its ticket, reset for the next.
    if (tk == a.n_items - 1) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_ticket = tk;
  }
  __syncthreads();
  const Item it = a.items[s_ticket];
  const TensorInfo ti = a.tinfo[it.tensor];

  if (it.kind == kResident) {  // one sub-chunk, x read once
    const bool full = (it.end - it.begin) == ES;
    float4 v[EV];
    if (full) load_f4<EV, true>(a.x, it.begin, it.end, v);
    else load_f4<EV, false>(a.x, it.begin, it.end, v);
    scale_f4<EV>(v, a);
    publish_partial(a, ti, it.tensor, it.chunk, sumsq_f4<EV>(v, 0.0f), sh);
    if (NORM_ONLY) return;
    const float norm = norm_wait_or_recompute<EV>(a, ti, it.tensor, sh);
    if (full) quant_store<WIDTH, HAS_U, true, EV>(v, a, it.begin, it.end, ti.begin, it.tensor, norm);
    else quant_store<WIDTH, HAS_U, false, EV>(v, a, it.begin, it.end, ti.begin, it.tensor, norm);
    return;
  }
  if (it.kind == kNorm) {
    publish_partial(a, ti, it.tensor, it.chunk, chunk_sumsq<EV>(a, it.begin, it.end), sh);
    return;
  }
  // kQuant: second pass of a large tensor.
  if (NORM_ONLY) return;
  const float norm = norm_wait_or_recompute<EV>(a, ti, it.tensor, sh);
  for (int64_t b = it.begin; b < it.end; b += ES)
    quant_sub<WIDTH, HAS_U, EV>(a, b, min(b + ES, it.end), ti.begin, it.tensor, norm);
}

template <int WIDTH, bool HAS_U, int V, bool NT>
__global__ __launch_bounds__(kThreads) void qsgd_quant_sub(EncArgs a) {
  // kSub / (V * 1024) blocks per 16 Ki item, V float4 per thread: 4 float4 (4 Ki-element
  // blocks) quantise 7 % faster than one 16 Ki block with 16 float4 per thread
  // (0.343 vs 0.368 ms on Llama-400M)
  constexpr int PER = (int)(kSub / ((int64_t)V * 1024));
  const Item it = a.items[blockIdx.x / PER];
  const int64_t b = it.begin + (int64_t)(blockIdx.x % PER) * V * 1024;
  if (b >= it.end) return;
  const TensorInfo ti = a.tinfo[it.tensor];
  const float norm = a.norm_in[it.tensor];
  if (it.chunk == 0 && blockIdx.x % PER == 0 && threadIdx.x == 0) a.norm_out[it.tensor] = norm;
  quant_sub<WIDTH, HAS_U, V, NT>(a, b, min(b + (int64_t)V * 1024, it.end), ti.begin, it.tensor, norm);
}

// ---------------------------------------------------------------- grid encoder (strategy 4)
// Small arenas (ResNet-18: 11 M elements in 2 976 blocks of 4 Ki): ONE launch of one 1024-thread
// workgroup per CU; each quarter (256 threads) holds kGridNB 4 Ki blocks of x in registers
// (the 16 wave partials of an item — 4 blocks x 4 waves — are summed in a fixed order in LDS and
// published as ONE fp64 item partial), every workgroup arrives at one grid-wide counter, and
// after it every tensor's norm is the same deterministic fold of its item partials in every
// workgroup (no second barrier; one round of loads per wave for tensors of <= 512 items) and the blocks are
// quantised from registers: x is read once, with no per-tensor hand-off chain (the ring's) and
// no sampled bracket (the bracketed encoder's four launches).  The hand-off is cdna_hip_
// programming.md §6 Guideline 16, table row 1: 8-byte sc1 partial stores, every wave's
// vmcnt(0), a workgroup barrier, one agent-scope add per workgroup; an sc1 poll of the counter,
// a workgroup barrier, sc1 loads; one workgroup per CU.  The counter wait is bounded (20 ms
// and a minimum number of polls); on expiry each workgroup recomputes the partials it needs
// from x in the producers' exact order (same bits) and sets err bit 2.
// (kGridNB 4 Ki blocks per quarter-workgroup per launch)

struct GridArgs {
  EncArgs e;                    // x, q, norm_out, alpha, fmt, levels, Philox key / offset, err, wait_ticks
  uint64_t* partials;           // fp64 bits, one per flat item (16 Ki elements)
  unsigned long long* bar;      // grid arrival counter (monotonic over launches)
  unsigned long long target;    // its value once every workgroup of this launch has arrived
  int64_t nblocks;              // 4 Ki blocks of the plan (4 per flat item)
  uint32_t dbg;                 // test hooks (omf_plan_set_debug spec bits): 32 arrive late, 64 no wait,
                                // 128 no fold, 256 no quantisation
};

typedef uint32_t g32x4_t __attribute__((ext_vector_type(4)));
// Range-checked buffer load of the float4 at byte offset voff of [base, base + bytes): dwords
// past the range read 0, so a tensor's partial last block needs no branch around its loads.
__device__ __forceinline__ float4 grid_ld4(const float* base, int64_t bytes, int voff) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, (int)max(bytes, (int64_t)0), 0x00020000);
  const g32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// Rows k = 0..3 of 4 Ki block [b, end) at quarter-thread lt: x * alpha (value format applied).
__device__ __forceinline__ void grid_load_block(const EncArgs& e, int64_t b, int64_t end, int lt, float4 (&v)[4]) {
  const float* base = e.x + b;
  const int64_t bytes = 4 * (end - b);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = grid_ld4(base, bytes, 16 * (k * kThreads + lt));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (e.alpha != 1.0f) {
      v[k] = mul4(v[k], e.alpha);
      if (e.fmt) v[k] = round_fmt4(v[k], e.fmt);
    }
  }
}

// The block's wave partial of quarter-thread lt's wave: the fp32 fma chain over its 16 values,
// then the fp64 wave butterfly (identical in the producer and in the recovery).
__device__ __forceinline__ double grid_partial(const float4 (&v)[4]) {
  return wave_sum_f64((double)sumsq_f4<4>(v, 0.0f));
}

// Item partial: its 16 wave partials (block q = 0..3 of the item, wave w = 0..3 of the block's
// quarter-workgroup) summed in fp64 in the order q-major, w-minor (producer and recovery alike).
// Tensor t's norm by ONE wave: lane l sums item partials l, l + 64, ... in order (fp64), then
// the butterfly — the same bits in every workgroup.  recover: the item partials are recomputed
// from x.
__device__ float grid_fold(const GridArgs& a, const Item* __restrict__ items, uint32_t p0, uint32_t pn, bool recover) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  if (!recover) {
    constexpr int U = 8;
    for (uint32_t j0 = 0; j0 < pn; j0 += 64 * U) {
      double d[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t j = j0 + 64 * u + lane;
        d[u] = j < pn ? __longlong_as_double((long long)ld_agent(&a.partials[p0 + j])) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j0 + 64 * u + lane < pn) s += d[u];
    }
  } else {  // each item partial as its workgroup made it
    for (uint32_t j = 0; j < pn; ++j) {
      const Item it = items[p0 + j];
      double ip = 0.0;
      for (int q = 0; q < 4; ++q) {
        const int64_t b = it.begin + (int64_t)q * kSpecBlk, end = min(b + kSpecBlk, it.end);
        for (int wq = 0; wq < 4; ++wq) {
          float4 v[4];
          grid_load_block(a.e, b, end, 64 * wq + lane, v);
          ip += grid_partial(v);
        }
      }
      if ((j & 63) == (uint32_t)lane) s += ip;
    }
  }
  return finish_norm(wave_sum_f64(s), a.e.fmt);
}

template <int WIDTH>
__global__ __launch_bounds__(1024) void qsgd_encode_grid(GridArgs a, const Item* __restrict__ items,
                                                         const int64_t* __restrict__ begins,
                                                         const uint32_t* __restrict__ pbeg,
                                                         const uint32_t* __restrict__ pcnt) {
  __shared__ float s_norm[kGridNB];
  __shared__ double s_part[kGridNB][16];
  __shared__ uint32_t s_ok;
  const EncArgs& e = a.e;
  const int lt = threadIdx.x & 255, qv = threadIdx.x >> 8, lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6, wq = wave & 3;
  const int64_t W = gridDim.x;
  float4 v[kGridNB][4];
  int64_t bb[kGridNB], be[kGridNB];
  int32_t tt[kGridNB];
  // phase 1: the blocks' x into registers, their wave partials published
#pragma unroll
  for (int i = 0; i < kGridNB; ++i) {
    const int64_t item = (int64_t)i * W + blockIdx.x;
    const bool live = 4 * item < a.nblocks;
    const Item it = items[live ? item : 0];
    bb[i] = it.begin + qv * kSpecBlk;
    be[i] = live ? min(bb[i] + kSpecBlk, it.end) : bb[i];  // empty range: loads read 0
    tt[i] = live ? it.tensor : -1;
    grid_load_block(e, bb[i], be[i], lt, v[i]);
  }
#pragma unroll
  for (int i = 0; i < kGridNB; ++i) {
    const double p = grid_partial(v[i]);
    if (lane == 0) s_part[i][4 * qv + wq] = p;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kGridNB; ++i)  // thread i: item i's partial, in a fixed order
    if ((int)threadIdx.x == i && tt[i] >= 0) {
      double ip = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) ip += s_part[i][j];
      st_agent(&a.partials[(int64_t)i * W + blockIdx.x], (uint64_t)__double_as_longlong(ip));
    }
  drain_vmem();
  __syncthreads();
  if (threadIdx.x == 0) {
    // (test hook dbg & 32: arrive only after the wait, so that every wait expires and the counter
    // still advances by the grid size per launch)
    if (!(a.dbg & 32u)) __hip_atomic_fetch_add(a.bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // bounded wait: wall clock AND a minimum number of polls (a queue context switch advances
    // the clock while the wave is saved)
    uint32_t ok = 1;
    if (!(a.dbg & 64u) && __hip_atomic_load(a.bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < a.target) {
      const uint64_t t0 = wall_clock64(), min_polls = e.wait_ticks >> 10;
      uint64_t polls = 0;
      for (int k = 0;; k = min(k + 1, 4)) {
        if (k < 2) __builtin_amdgcn_s_sleep(2);
        else __builtin_amdgcn_s_sleep(16);
        if (__hip_atomic_load(a.bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.target) break;
        if (++polls > min_polls && wall_clock64() - t0 > e.wait_ticks) {
          ok = 0;
          __hip_atomic_fetch_or(e.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
    if (a.dbg & 32u) __hip_atomic_fetch_add(a.bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_ok = ok;
  }
  __syncthreads();
  // phase 2: wave i folds the norm of iteration i's tensor (the quarters of one item share it)
  if (wave < kGridNB && tt[wave] >= 0) {
    const int32_t t = tt[wave];
    const uint32_t p0 = pbeg[t];
    const float norm = (a.dbg & 128u) ? 1.0f : grid_fold(a, items, p0, pcnt[t], s_ok == 0u);
    if (lane == 0) {
      s_norm[wave] = norm;
      if ((int64_t)wave * W + blockIdx.x == (int64_t)p0) e.norm_out[t] = norm;  // the tensor's first item
    }
  }
  __syncthreads();
  // phase 3: levels from registers
  if (a.dbg & 256u) return;
#pragma unroll
  for (int i = 0; i < kGridNB; ++i) {
    if (tt[i] < 0 || bb[i] >= be[i]) continue;
    const float norm = s_norm[i];
    const Divisor dv(norm, e.fmt);
    float4 uu[4];
    {
      const uint64_t G = (uint64_t)((bb[i] - begins[tt[i]]) >> 12) * (uint64_t)kThreads + (uint64_t)lt;
      uint32_t w[12];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint64_t ctr = 3 * G + c;
        const uint4 r = philox4x32_10(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)tt[i], e.offset),
                                      e.seed_lo, e.seed_hi);
        w[4 * c] = r.x; w[4 * c + 1] = r.y; w[4 * c + 2] = r.z; w[4 * c + 3] = r.w;
      }
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) uu[sl] = u24x4(w[3 * sl], w[3 * sl + 1], w[3 * sl + 2]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t el = bb[i] + 4 * ((int64_t)k * kThreads + lt);
      if (el >= be[i]) continue;
      int32_t qq[4];
      qsgd_quad<false>(v[i][k], uu[k], dv, e.levels, !(norm != 0.0f), qq);
      store_quad<WIDTH>(e, el, be[i], qq);
    }
  }
}

// dst = src / d (DIV) or src over the plan's flat items: the tensors' elements only, so the padding
// between tensors is neither read nor written.  dst may be src.  Item starts are multiples of 4.
template <bool DIV>
__global__ __launch_bounds__(kThreads) void items_f32_kernel(const Item* __restrict__ items, const float* src, float* dst,
                                                             float d) {
  const Item it = items[blockIdx.x];
  for (int64_t e = it.begin + 4 * (int64_t)threadIdx.x; e < it.end; e += 4 * kThreads) {
    if (e + 4 <= it.end) {
      float4 v = *reinterpret_cast<const float4*>(src + e);
      if (DIV) { v.x = v.x / d; v.y = v.y / d; v.z = v.z / d; v.w = v.w / d; }
      *reinterpret_cast<float4*>(dst + e) = v;
    } else {
      for (int64_t i = e; i < it.end; ++i) dst[i] = DIV ? src[i] / d : src[i];
    }
  }
}

}  // namespace

// ====================================================================== host side
// struct omf_plan and its stream ordering (plan_enter / plan_leave) are in omf_plan.h; the work-item
// tables, the carve of a device allocation and the encoder choice in omf_plan_layout.h.

// Allocates a carve's bytes into *block, binds its pointers and fills its regions.  On failure *block
// and every pointer of the carve are NULL.
static int make_block(const Carve& c, void** block) {
  auto fill = [&]() -> int {
    OMF_HIP(hipMalloc(block, c.bytes()));
    for (const Carve::Region& r : c.regions()) {
      void* dst = static_cast<uint8_t*>(*block) + r.offset;
      if (!r.bytes) continue;
      if (r.src) OMF_HIP(hipMemcpy(dst, r.src, r.bytes, hipMemcpyHostToDevice));
      else if (r.zero) OMF_HIP(hipMemset(dst, 0, r.bytes));
    }
    return OMF_OK;
  };
  const int rc = fill();
  if (rc != OMF_OK && *block) {
    (void)hipFree(*block);
    *block = nullptr;
  }
  c.bind(*block);
  return rc;
}

// (Re)build every table (omf_plan_layout.cpp) and upload them into one device allocation.  Each
// region is declared once, in the allocation's order: its pointer, element count and contents.
static int upload_plan(omf_plan* p) {
  const ring::Config rc = ring::config(p->ring_cfg);
  Desc d;
  d.sizes = p->sizes.data();
  d.offsets = p->offsets.data();
  d.nt = p->nt;
  d.chunk = p->chunk;
  d.ev = p->ev;
  d.cap = p->cap;
  d.ring_chunk = ring::chunk_elems(rc);
  d.ring_slots = rc.slots;
  d.ring_kind = rc.kind;
  d.ring_grid = p->ring_grid;
  d.ring_big_mode = p->ring_big_mode;
  d.ring_gap = p->ring_gap;
  d.ring_hold_override = p->ring_hold_override;
  Tables tb;
  if (!build_tables(d, tb)) return fail(OMF_EINVAL, "too many work items");
  p->n_enc[0] = tb.n_enc[0];
  p->n_enc[1] = tb.n_enc[1];
  p->n_flat = tb.n_flat;
  p->n_partials = tb.n_partials;
  p->n_ring = (int64_t)tb.ring.size();
  p->n_ring_gran = tb.n_ring_gran;
  p->ring_hold_max = tb.ring_hold_max;
  p->ring_two_pass = tb.ring_two_pass;
  p->n_spec_blocks = tb.n_spec_blocks;
  p->n_spec_fold = (int64_t)tb.fold_items.size();
  p->n_dec_blocks = (int64_t)tb.dec_binfo.size();
  p->off_counters = 16;
  p->off_gran = round16(p->off_counters + 4 * (size_t)p->nt);
  p->sync_bytes = round16(p->off_gran + 8 * (size_t)p->nt);
  const size_t nt = (size_t)p->nt, nb = (size_t)p->n_spec_blocks;
  Carve c;
  c.zero(p->d_sync, p->sync_bytes);  // first: its per-call memset is 16-byte aligned and sized
  c.copy(p->d_enc[0], tb.enc[0]);
  c.copy(p->d_enc[1], tb.enc[1]);
  c.copy(p->d_flat, tb.flat);
  c.copy(p->d_tinfo[0], tb.tinfo[0]);
  c.copy(p->d_tinfo[1], tb.tinfo[1]);
  c.raw(p->d_partials, (size_t)p->n_partials);
  c.copy(p->d_sizes, p->sizes);
  c.copy(p->d_begins, p->offsets);
  c.copy(p->d_ring, tb.ring);
  c.copy(p->d_ring_t, tb.ring_t);
  c.zero(p->d_ring_gran, (size_t)p->n_ring_gran);  // epoch 0 is never a launch's tag
  c.zero(p->d_ring_prof, 16);
  c.copy(p->d_spec_br_items, tb.br_items);
  c.copy(p->d_spec_fold_items, tb.fold_items);
  c.raw(p->d_spec_seg_part, tb.fold_items.size());
  c.zero(p->d_spec_cnt, nt + 1);
  c.raw(p->d_spec_br, nt);
  c.zero(p->d_spec_ngran, nt);  // epoch 0 is never a launch's tag
  c.raw(p->d_spec_part, kWaves * nb);
  c.raw(p->d_spec_slots, kSpecSlot * nb);
  c.raw(p->d_spec_heads, kWaves * nb);
  c.copy(p->d_dec_binfo, tb.dec_binfo);
  c.raw(p->d_spec_recs, 2 * (size_t)kWaves * kSpecPerWave * nb);
  c.zero(p->d_spec_flags, nt);
  c.zero(p->d_spec_status, nt);  // spec_stats reads them before any encode
  c.copy(p->d_grid_pbeg, tb.grid_pbeg);
  c.copy(p->d_grid_pcnt, tb.grid_pcnt);
  c.zero(p->d_grid_bar, 2);
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  if (p->d_block) {
    OMF_HIP(hipDeviceSynchronize());
    (void)hipFree(p->d_block);
    p->d_block = nullptr;
  }
  p->grid_launches = 0;
  return make_block(c, &p->d_block);
}

// The buffers of a group made at the first encode that needs it: the regions declared in `c`, each
// an allocation of its own (the fused bracket's counters and granules carved out of one allocation
// with its sums, pages apart before, cost the Llama-400M s = 4 encode 0.342 against 0.330 ms:
// profiles/r08_plan_host_ab.txt), zero fills on `st`.  The plan owns them (d_lazy); on failure
// none is kept and every pointer of the group is NULL.
int omf::make_buffers(omf_plan* p, const Carve& c, hipStream_t st) {
  std::vector<void*> made;
  auto alloc = [&]() -> int {
    for (const Carve::Region& r : c.regions()) {
      void* d = nullptr;
      OMF_HIP(hipMalloc(&d, r.bytes));
      made.push_back(d);
      if (r.zero) OMF_HIP(hipMemsetAsync(d, 0, r.bytes, st));
    }
    return OMF_OK;
  };
  if (const int rc = alloc()) {
    for (void* d : made) (void)hipFree(d);
    c.bind(nullptr);
    return rc;
  }
  for (size_t i = 0; i < made.size(); ++i) c.regions()[i].set(c.regions()[i].field, made[i]);
  p->d_lazy.insert(p->d_lazy.end(), made.begin(), made.end());
  return OMF_OK;
}

extern "C" {

int omf_plan_create(const int64_t* sizes, const int64_t* offsets, int32_t ntensors, int64_t chunk_elems, int device,
                    omf_plan** out) {
  if (!out) return fail(OMF_EINVAL, "omf_plan_create: out is NULL");
  *out = nullptr;
  if (ntensors <= 0 || !sizes || !offsets) return fail(OMF_EINVAL, "omf_plan_create: need >= 1 tensor");
  if (ntensors >= (1 << 24)) return fail(OMF_EINVAL, "omf_plan_create: at most 2^24 - 1 tensors");
  if (chunk_elems == 0) chunk_elems = 2 * kSub;  // two-pass encode items: 128 KiB of fp32 (32 Ki: 0.579 vs
                                                 // 0.595 ms at 64 Ki on Llama-400M, scripts/exp/ab_chunk.py)
  if (chunk_elems < kSub || chunk_elems % kSub != 0)
    return fail(OMF_EINVAL, "omf_plan_create: chunk_elems must be a positive multiple of 16384");
  for (int32_t t = 0; t < ntensors; ++t) {
    if (sizes[t] <= 0 || offsets[t] < 0 || (offsets[t] & 3))
      return fail(OMF_EINVAL, "omf_plan_create: tensor " + std::to_string(t) +
                                  ": size must be > 0 and offset a non-negative multiple of 4");
    if (t > 0 && offsets[t] < offsets[t - 1] + sizes[t - 1])
      return fail(OMF_EINVAL, "omf_plan_create: tensors must be ordered and non-overlapping");
  }
  auto* p = new (std::nothrow) omf_plan();
  if (!p) return fail(OMF_ENOMEM, "omf_plan_create: host allocation failed");
  p->device = device;
  p->nt = ntensors;
  p->chunk = chunk_elems;
  p->sizes.assign(sizes, sizes + ntensors);
  p->offsets.assign(offsets, offsets + ntensors);
  p->arena_end = offsets[ntensors - 1] + sizes[ntensors - 1];
  p->spec_last_pw = kSpecPerWave;
  {
    // Co-resident capacity of the encoder (occupancy x CUs over every instantiation); a
    // tensor takes the register-resident path only with half of it as margin.
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    if (!g.ok || hipGetDeviceProperties(&prop, device) != hipSuccess) {
      delete p;
      return fail(OMF_EHIP, "omf_plan_create: cannot query the device");
    }
    if (const char* ev = omf::knob("OMF_ENCODE_ROWS")) p->ev = atoi(ev) == 16 ? 16 : 8;  // tuning knob
    const void* k16[5] = {(const void*)qsgd_encode_ordered<1, false, false, 16>,
                          (const void*)qsgd_encode_ordered<1, true, false, 16>,
                          (const void*)qsgd_encode_ordered<4, false, false, 16>,
                          (const void*)qsgd_encode_ordered<4, true, false, 16>,
                          (const void*)qsgd_encode_ordered<1, false, true, 16>};
    const void* k8[5] = {(const void*)qsgd_encode_ordered<1, false, false, 8>,
                         (const void*)qsgd_encode_ordered<1, true, false, 8>,
                         (const void*)qsgd_encode_ordered<4, false, false, 8>,
                         (const void*)qsgd_encode_ordered<4, true, false, 8>,
                         (const void*)qsgd_encode_ordered<1, false, true, 8>};
    const void* const* kerns = p->ev == 8 ? k8 : k16;
    int nb_min = 1 << 30;
    for (int i = 0; i < 5; ++i) {
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kerns[i], kThreads, 0) != hipSuccess || nb < 1) nb = 1;
      nb_min = std::min(nb_min, nb);
    }
    p->cap = std::max<int64_t>(1, (int64_t)nb_min * prop.multiProcessorCount / 2);
    // Ring encoder: configuration and grid (tuning knobs for experiments only).
    if (const char* rc = omf::knob("OMF_RING_CFG")) p->ring_cfg = std::max(0, std::min(atoi(rc), omf::ring::num_configs() - 1));
    if (const char* bm = omf::knob("OMF_RING_BIG")) p->ring_big_mode = atoi(bm) == 1 ? 1 : 0;
    if (const char* gp = omf::knob("OMF_RING_GAP")) p->ring_gap = atoll(gp);
    // Switches that change what an encode writes (skipped launches, no quantisation) are never
    // read from the environment of a release build: tests set them per plan (omf_plan_set_debug);
    // experiment builds (-DOMF_EXPERIMENTS, scripts/exp/build_variants.sh) also take them here.
#ifdef OMF_EXPERIMENTS
    if (const char* dg = omf::knob("OMF_RING_DBG")) p->ring_dbg = (uint32_t)atoi(dg);
    if (const char* sk = omf::knob("OMF_SPEC_SKIP")) p->spec_skip = (uint32_t)atoi(sk);
#endif
    if (const char* zs = omf::knob("OMF_SPEC_ZSIG")) p->spec_zsig = p->spec_zsig_wide = std::max(1.0f, (float)atof(zs));
    // Default strategy by arena size: the bracketed single-read encoder from 2^25 elements
    // (Llama-400M 0.386 ms against the two-pass 0.59 and the ring 0.63; Llama-150M 0.25 against
    // 0.35), the ring below (ResNet-18: 0.032 ms against 0.08 for the bracket's four launches).
    p->strategy = p->arena_end >= ((int64_t)1 << 25) ? 3 : 2;
    if (const char* st = omf::knob("OMF_ENCODE_STRATEGY")) p->strategy = std::max(0, std::min(atoi(st), 4));
    if (const char* sw = omf::knob("OMF_SPEC_WIDE")) p->spec_wide = atoi(sw) != 0 ? 1 : 0;
    if (const char* fb = omf::knob("OMF_SPEC_FB")) p->spec_fb = atoi(fb) != 0 ? 1 : 0;
    {  // grid encoder: one 1024-thread workgroup per CU must fit
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)qsgd_encode_grid<1>, 1024, 0) == hipSuccess &&
          nb >= 1)
        p->grid_wgs = prop.multiProcessorCount;
    }
    p->ring_grid = omf::ring::grid_size(p->ring_cfg, device);
    if (p->ring_grid <= 0) {
      delete p;
      return fail(OMF_EHIP, "omf_plan_create: cannot size the ring encoder grid");
    }
  }
  if (int r = upload_plan(p)) {
    if (p->d_block) (void)hipFree(p->d_block);
    delete p;
    return r;
  }
  *out = p;
  return OMF_OK;
}

int omf_plan_destroy(omf_plan* plan) {
  if (!plan) return OMF_OK;
  DeviceGuard g(plan->device);
  if (plan->last_ev) (void)hipEventDestroy(plan->last_ev);
  if (plan->d_block) (void)hipFree(plan->d_block);
  for (void* d : plan->d_lazy)
    if (d) (void)hipFree(d);
  for (auto& e : plan->topk_tables) (void)hipFree(e.dev);
  delete plan;
  return OMF_OK;
}

int64_t omf_plan_encode_items(const omf_plan* plan) {
  if (!plan) return -1;
  switch (plan->strategy) {  // of the strategy's own encoder
    case kEncBracket: return plan->n_spec_blocks;
    case kEncGrid: return plan->grid_wgs;
    case kEncRing: return plan->n_ring;
    default: return plan->n_enc[plan->strategy];
  }
}

int32_t omf_plan_encode_strategy(const omf_plan* plan) { return plan ? plan->strategy : -1; }
int32_t omf_plan_last_encoder(const omf_plan* plan) { return plan ? plan->last_encoder : -1; }
int omf_plan_set_fused_bracket(omf_plan* plan, int32_t on) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  plan->spec_fb = on != 0 ? 1 : 0;
  return OMF_OK;
}
int omf_plan_set_wide_levels(omf_plan* plan, int32_t on) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  plan->spec_wide = on != 0 ? 1 : 0;
  return OMF_OK;
}

int omf_plan_set_encode_strategy(omf_plan* plan, int32_t strategy) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (strategy < 0 || strategy > 4)
    return fail(OMF_EINVAL, "strategy must be 0 (resident), 1 (two-pass), 2 (single-read ring), 3 (bracketed "
                            "single-read) or 4 (grid)");
  plan->strategy = strategy;
  return OMF_OK;
}

int64_t omf_plan_resident_capacity(const omf_plan* plan) { return plan ? plan->cap : -1; }

int omf_plan_set_ring(omf_plan* plan, int32_t cfg, int32_t big_mode, int64_t gap, int64_t hold_max) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (cfg >= omf::ring::num_configs() || cfg < -1) return fail(OMF_EINVAL, "omf_plan_set_ring: bad configuration");
  if (big_mode < -1 || big_mode > 1 || gap < -2 || hold_max < -1)
    return fail(OMF_EINVAL, "omf_plan_set_ring: bad arguments");
  if (cfg >= 0 && cfg != plan->ring_cfg) {
    DeviceGuard g(plan->device);
    const int grid = omf::ring::grid_size(cfg, plan->device);
    if (grid <= 0) return fail(OMF_EHIP, "omf_plan_set_ring: cannot size the grid");
    plan->ring_cfg = cfg;
    plan->ring_grid = grid;
  }
  if (big_mode >= 0) plan->ring_big_mode = big_mode;
  if (gap >= -1) plan->ring_gap = gap;
  if (hold_max >= 0) plan->ring_hold_override = hold_max;
  return upload_plan(plan);
}

int omf_plan_ring_profile(omf_plan* plan, int64_t* out16) {
  if (!plan || !out16) return fail(OMF_EINVAL, "omf_plan_ring_profile: NULL argument");
  DeviceGuard g(plan->device);
  OMF_HIP(hipDeviceSynchronize());
  OMF_HIP(hipMemcpy(out16, plan->d_ring_prof, 8 * 16, hipMemcpyDeviceToHost));
  OMF_HIP(hipMemset(plan->d_ring_prof, 0, 8 * 16));
  return OMF_OK;
}

int omf_plan_ring_info(const omf_plan* plan, int64_t* out) {
  if (!plan || !out) return fail(OMF_EINVAL, "omf_plan_ring_info: NULL argument");
  out[0] = plan->ring_grid;
  out[1] = omf::ring::chunk_elems(omf::ring::config(plan->ring_cfg));
  out[2] = plan->n_ring;
  out[3] = plan->ring_hold_max;
  out[4] = plan->ring_two_pass;
  out[5] = plan->ring_cfg;
  return OMF_OK;
}

int omf_plan_set_resident_capacity(omf_plan* plan, int64_t cap, int64_t wait_us) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (cap < 0 || wait_us < 0) return fail(OMF_EINVAL, "cap and wait_us must be >= 0");
  if (cap > 0) plan->cap = cap;
  plan->wait_ticks = wait_us > 0 ? (uint64_t)wait_us * 100ull : kWaitTicks;
  if (cap > 0) return upload_plan(plan);
  return OMF_OK;
}

int omf_plan_set_debug(omf_plan* plan, uint32_t ring_dbg, uint32_t spec_dbg, int64_t lds_wait_us) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (lds_wait_us < 0) return fail(OMF_EINVAL, "lds_wait_us must be >= 0");
  if ((ring_dbg & ~15u) || (spec_dbg & ~511u)) return fail(OMF_EINVAL, "omf_plan_set_debug: unknown switch bits");
  plan->ring_dbg = ring_dbg;
  plan->spec_skip = spec_dbg;
  plan->lds_wait_ticks = lds_wait_us > 0 ? (uint64_t)lds_wait_us * 100ull : kWaitTicks;
  return OMF_OK;
}

int omf_plan_spec_stats(omf_plan* plan, void* stream, int64_t* out4) {
  if (!plan || !out4) return fail(OMF_EINVAL, "omf_plan_spec_stats: NULL argument");
  DeviceGuard g(plan->device);
  OMF_HIP(hipStreamSynchronize((hipStream_t)stream));
  std::vector<uint32_t> status(plan->nt), heads((size_t)kWaves * (size_t)plan->n_spec_blocks);
  std::vector<SpecBracket> br(plan->nt);
  OMF_HIP(hipMemcpy(status.data(), plan->d_spec_status, 4 * (size_t)plan->nt, hipMemcpyDeviceToHost));
  OMF_HIP(hipMemcpy(br.data(), plan->d_spec_br, sizeof(SpecBracket) * (size_t)plan->nt, hipMemcpyDeviceToHost));
  OMF_HIP(hipMemcpy(heads.data(), plan->d_spec_heads, 4 * heads.size(), hipMemcpyDeviceToHost));
  int64_t whole = 0, deferred = 0, listed = 0, full = 0;
  for (int32_t t = 0; t < plan->nt; ++t) {
    whole += status[t] != 0u;
    deferred += br[t].mode != 0u;
  }
  for (int64_t blk = 0; blk < plan->n_spec_blocks; ++blk)
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t c = heads[(size_t)blk * kWaves + w] & 0xffu;
      listed += c;
      full += c == (uint32_t)plan->spec_last_pw;
    }
  out4[0] = whole;
  out4[1] = deferred;
  out4[2] = listed;
  out4[3] = full;
  return OMF_OK;
}

int omf_plan_check(omf_plan* plan, void* stream) {
  if (!plan) return fail(OMF_EINVAL, "omf_plan_check: plan is NULL");
  DeviceGuard g(plan->device);
  OMF_HIP(hipStreamSynchronize((hipStream_t)stream));
  // the plan's launches on this stream are complete: a later call on another stream needs no
  // ordering against it (and the stream may now be destroyed)
  if (plan->last_valid && plan->last_stream == (hipStream_t)stream) plan->last_valid = false;
  uint32_t err = 0;
  OMF_HIP(hipMemcpy(&err, plan->err_word(), 4, hipMemcpyDeviceToHost));
  if (err) OMF_HIP(hipMemset(plan->err_word(), 0, 4));  // report each event once
  if (err & 4u)
    return fail(OMF_ETIMEOUT, "QSGD encoder: an on-chip wait exceeded its bound (a ring hand-off, or a "
                              "bracketed-encoder fix waiting for its tensor's norm) and was abandoned; the "
                              "payload of that launch is invalid");
  if (err & 8u)
    return fail(OMF_ETIMEOUT, "Top-K encoder: a grid barrier of the exact tail (the device-side fallback) "
                              "exceeded its bound and was abandoned; the selection of that call is invalid");
  if (err & 2u) {
    set_error("encoder recomputed a norm after a bounded wait (items not co-resident); results are exact");
    return 1;
  }
  set_error("");
  return OMF_OK;
}

}  // extern "C"

static int check_bits(int32_t s) {
  if (s < 0 || s > 30) return fail(OMF_EINVAL, "bit_width must be in [0, 30] (levels = 2^bit_width is an int32 on the wire)");
  return OMF_OK;
}

// The choice function's view of a call on plan `p` (omf_plan_layout.h).
static Call call_of(const omf_plan* p, int32_t s, bool caller_u, bool caller_norms, bool norms_only, uint32_t fmt,
                    bool divide, bool last_client) {
  Call c;
  c.strategy = p->strategy;
  c.bits = s;
  c.caller_u = caller_u;
  c.caller_norms = caller_norms;
  c.norms_only = norms_only;
  c.fmt = fmt;
  c.divide = divide;
  c.last_client = last_client;
  c.wide_levels = p->spec_wide != 0;
  c.fused_bracket = p->spec_fb != 0;
  c.spec_dbg = p->spec_skip;
  c.grid_fits = p->grid_wgs > 0 && p->n_spec_blocks <= (int64_t)p->grid_wgs * 4 * kGridNB;
  return c;
}

using EncKernel = void (*)(EncArgs);

// Norms supplied by the caller: one pass over the flat items, 4 blocks of 4 Ki elements per 16 Ki item.
static void launch_caller_norms(omf_plan* p, const EncCall& c) {
  static const EncKernel kern[2][2] = {  // [int32 wire][caller uniforms]
      {qsgd_quant_sub<1, false, 4, false>, qsgd_quant_sub<1, true, 4, false>},
      {qsgd_quant_sub<4, false, 4, false>, qsgd_quant_sub<4, true, 4, false>}};
  EncArgs a = enc_args(p, c);
  a.items = p->d_flat;
  a.tinfo = p->d_tinfo[0];
  launch_kernel(kern[c.width == 4][c.u != nullptr], dim3((unsigned)(p->n_flat * 4)), dim3(kThreads), 0, c.st, a);
}

// Grid encoder (strategy 4): one launch of one workgroup per CU.
static int launch_grid(omf_plan* p, const EncCall& c) {
  GridArgs ga;
  ga.e = enc_args(p, c);
  ga.e.items = p->d_flat;
  ga.partials = p->d_spec_part;
  ga.bar = p->d_grid_bar;
  ga.target = (unsigned long long)(p->grid_launches + 1) * (unsigned long long)p->grid_wgs;
  ga.nblocks = p->n_spec_blocks;
  ga.dbg = p->spec_skip;
  launch_kernel(c.width == 1 ? qsgd_encode_grid<1> : qsgd_encode_grid<4>, dim3((unsigned)p->grid_wgs), dim3(1024), 0, c.st, ga,
         p->d_flat, p->d_begins, p->d_grid_pbeg, p->d_grid_pcnt);
  OMF_HIP(hipGetLastError());
  // counted only once the launch is in: the device's monotonic arrival counter advances by
  // grid_wgs per launch that ran, so a failed launch must not move the host's target
  ++p->grid_launches;
  return OMF_OK;
}

// Single-read ring (omf_qsgd_ring.hip): also the fused PS step's divide + encode in one launch.
static int launch_ring(omf_plan* p, const EncCall& c) {
  omf::ring::Args r;
  r.x = c.x; r.u = c.u; r.q = c.q; r.norm_out = c.norm_out;
  r.items = p->d_ring; r.tinfo = p->d_ring_t; r.gran = p->d_ring_gran;
  r.err = p->err_word();
  r.n_items = p->n_ring;
  r.alpha = c.alpha;
  r.fmt = c.fmt;
  r.round_in = (c.fmt != 0 && c.alpha != 1.0f) ? 1u : 0u;
  r.divisor = c.divisor;
  r.divide = c.divisor != 0.0f ? 1u : 0u;
  r.xout = c.xout;
  r.levels = (float)(1u << c.s);
  r.seed_lo = (uint32_t)c.seed; r.seed_hi = (uint32_t)(c.seed >> 32); r.offset = (uint32_t)c.offset;
  if (++p->ring_epoch == 0) ++p->ring_epoch;
  r.epoch = p->ring_epoch;
  r.wait_ticks = p->wait_ticks;
  r.lds_wait_ticks = p->lds_wait_ticks;
  r.dbg = p->ring_dbg;
  r.prof = p->d_ring_prof;
  const int grid = (int)std::min<int64_t>(p->ring_grid, std::max<int64_t>(p->n_ring, 1));
  if (omf::ring::launch(p->ring_cfg, c.width, c.u != nullptr, r, grid, c.st) != 0)
    return fail(OMF_EHIP, "ring encoder launch failed");
  return OMF_OK;
}

// Ticket-ordered launch over sequence `strat` (0: register-resident + two-pass, 1: two-pass), and
// every norms-only pass.  No per-call memset: tickets and arrival counters are reset in-kernel by
// their last user, and granules carry this launch's epoch.
static void launch_ordered(omf_plan* p, const EncCall& c, int strat) {
  static const EncKernel kern[2][5] = {  // [16 rows per thread][norms only, or 1 + 2 x int32 wire + caller uniforms]
      {qsgd_encode_ordered<1, false, true, 8>, qsgd_encode_ordered<1, false, false, 8>, qsgd_encode_ordered<1, true, false, 8>,
       qsgd_encode_ordered<4, false, false, 8>, qsgd_encode_ordered<4, true, false, 8>},
      {qsgd_encode_ordered<1, false, true, 16>, qsgd_encode_ordered<1, false, false, 16>, qsgd_encode_ordered<1, true, false, 16>,
       qsgd_encode_ordered<4, false, false, 16>, qsgd_encode_ordered<4, true, false, 16>}};
  EncArgs a = enc_args(p, c);
  if (++p->epoch == 0) ++p->epoch;
  a.epoch = p->epoch;
  a.n_items = (uint32_t)p->n_enc[strat];
  a.items = p->d_enc[strat];
  a.tinfo = p->d_tinfo[strat];
  const int k = c.norm_only ? 0 : 1 + 2 * (c.width == 4) + (c.u != nullptr);
  launch_kernel(kern[p->ev != 8][k], dim3((unsigned)p->n_enc[strat]), dim3(kThreads), 0, c.st, a);
}

static int encode_launch(omf_plan* p, EncCall c) {
  if (int r = check_bits(c.s)) return r;
  c.width = (1 << c.s) <= 127 ? 1 : 4;
  if (!c.x || !c.norm_out || (!c.norm_only && !c.q)) return fail(OMF_EINVAL, "x, q and norm_out must be non-NULL");
  if (!aligned(c.x, 16) || (c.u && !aligned(c.u, 16)) || (c.q && !aligned(c.q, c.width == 1 ? 4 : 16)))
    return fail(OMF_EINVAL, "misaligned buffer (fp32/int32 need 16 B, int8 needs 4 B alignment)");
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  const Choice ch = choose_encoder(call_of(p, c.s, c.u != nullptr, c.norm_in != nullptr, c.norm_only, c.fmt,
                                           c.divisor != 0.0f, c.acc_in != nullptr));
  if (!c.norm_only) p->last_encoder = ch.encoder;
  switch (ch.encoder) {
    case kEncCallerNorms: launch_caller_norms(p, c); break;
    case kEncGrid: return launch_grid(p, c);
    case kEncBracket: return bracket::launch(p, c, ch);
    case kEncRing:
      if (int r = launch_ring(p, c)) return r;
      break;
    case kEncResident:
    case kEncOrdered: launch_ordered(p, c, ch.encoder); break;
  }
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

static int encode_impl(omf_plan* p, const float* x, float alpha, int32_t s, const float* u, uint64_t seed,
                       uint64_t offset, const float* norm_in, void* q, float* norm_out, bool norm_only, void* stream,
                       float divisor = 0.0f, float* xout = nullptr, int32_t fmt = 0, const AccIn* acc_in = nullptr) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  if (fmt < 0 || fmt > 2) return fail(OMF_EINVAL, "value_format must be 0 (fp32), 1 (bf16) or 2 (fp16)");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const hipStream_t st = (hipStream_t)stream;
  if (int r = plan_enter(p, st)) return r;
  if (int r = encode_launch(p, EncCall{x, alpha, s, u, seed, offset, norm_in, q, norm_out, norm_only, st, divisor, xout,
                                       (uint32_t)fmt, acc_in, 0}))
    return r;
  return plan_leave(p, st);
}

extern "C" {

int omf_qsgd_encode(omf_plan* plan, const float* x, float alpha, int32_t bit_width, const float* u, uint64_t seed,
                    uint64_t offset, const float* norm_in, void* q_out, float* norm_out, void* stream) {
  return encode_impl(plan, x, alpha, bit_width, u, seed, offset, norm_in, q_out, norm_out, false, stream);
}

int omf_qsgd_encode_ex(omf_plan* plan, const float* x, float alpha, int32_t bit_width, int32_t value_format,
                       const float* u, uint64_t seed, uint64_t offset, const float* norm_in, void* q_out,
                       float* norm_out, void* stream) {
  return encode_impl(plan, x, alpha, bit_width, u, seed, offset, norm_in, q_out, norm_out, false, stream, 0.0f,
                     nullptr, value_format);
}

int omf_qsgd_norms_ex(omf_plan* plan, const float* x, float alpha, int32_t value_format, float* norm_out,
                      void* stream) {
  return encode_impl(plan, x, alpha, 0, nullptr, 0, 0, nullptr, nullptr, norm_out, true, stream, 0.0f, nullptr,
                     value_format);
}

int omf_ps_apply_encode(omf_plan* p, const float* acc, float divisor, float* avg_out, int32_t bit_width,
                        const float* u, uint64_t seed, uint64_t offset, void* q_out, float* norm_out, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  if (!acc || !avg_out) return fail(OMF_EINVAL, "omf_ps_apply_encode: acc and avg_out must be non-NULL");
  if (!(divisor != 0.0f)) return fail(OMF_EINVAL, "omf_ps_apply_encode: divisor must be non-zero");
  if (!aligned(avg_out, 16)) return fail(OMF_EINVAL, "omf_ps_apply_encode: avg_out must be 16-byte aligned");
  const size_t bytes = 4 * (size_t)p->arena_end;
  const bool alias = avg_out == acc;
  if (!alias && overlaps(acc, bytes, avg_out, bytes))
    return fail(OMF_EINVAL, "omf_ps_apply_encode: avg_out partially overlaps acc (pass the same pointer or disjoint buffers)");
  // The fused launch reads acc while it writes avg (second-pass chunks of large tensors
  // re-read acc, the bounded-wait fallback recomputes partials from it), so it needs
  // avg_out disjoint from acc; in place it runs as divide + encode.
  if (!alias)  // one ring launch: read acc once, write avg and the payload
    return encode_impl(p, acc, 1.0f, bit_width, u, seed, offset, nullptr, q_out, norm_out, false, stream, divisor,
                       avg_out);
  // in place: the same results as divide, then encode (the tensors' elements only: the padding
  // between them stays as the caller left it)
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  if (p->n_flat > 0) {
    hipLaunchKernelGGL(items_f32_kernel<true>, dim3((unsigned)p->n_flat), dim3(kThreads), 0, (hipStream_t)stream,
                       (const Item*)p->d_flat, (const float*)avg_out, avg_out, divisor);
    OMF_HIP(hipGetLastError());
  }
  return encode_impl(p, avg_out, 1.0f, bit_width, u, seed, offset, nullptr, q_out, norm_out, false, stream);
}

int omf_ps_accumulate_apply_encode(omf_plan* p, const float* acc, const void* q_in, int32_t width_in,
                                   int32_t levels_in, const float* norm_in, float* acc_out, float divisor,
                                   float* avg_out, int32_t bit_width, const float* u, uint64_t seed, uint64_t offset,
                                   void* q_out, float* norm_out, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  if (!acc || !avg_out || !q_in || !norm_in)
    return fail(OMF_EINVAL, "omf_ps_accumulate_apply_encode: acc, q_in, norm_in and avg_out must be non-NULL");
  if (width_in != 8 && width_in != 32) return fail(OMF_EINVAL, "width_in must be 8 or 32");
  if (levels_in <= 0) return fail(OMF_EINVAL, "levels_in must be > 0");
  if (!(divisor != 0.0f)) return fail(OMF_EINVAL, "omf_ps_accumulate_apply_encode: divisor must be non-zero");
  if (int r = check_bits(bit_width)) return r;
  if (!aligned(acc, 16) || !aligned(avg_out, 16) || (acc_out && !aligned(acc_out, 16)) ||
      !aligned(q_in, width_in == 8 ? 4 : 16))
    return fail(OMF_EINVAL, "misaligned buffer (fp32/int32 need 16 B, int8 needs 4 B alignment)");
  const size_t bytes = 4 * (size_t)p->arena_end;
  auto overlap = [bytes](const void* x, const void* y) { return overlaps(x, bytes, y, bytes); };
  if (overlap(avg_out, acc) || (acc_out && overlap(avg_out, acc_out)) || (acc_out && acc_out != acc && overlap(acc_out, acc)))
    return fail(OMF_EINVAL, "omf_ps_accumulate_apply_encode: avg_out must be disjoint from acc and acc_out; acc_out is "
                            "acc itself or disjoint from it");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  // one pass (acc and the last payload read once) where the bracketed encoder serves the call
  if (choose_encoder(call_of(p, bit_width, u != nullptr, false, false, 0u, true, true)).encoder == kEncBracket) {
    const AccIn ai{q_in, width_in, levels_in, norm_in, acc_out};
    return encode_impl(p, acc, 1.0f, bit_width, u, seed, offset, nullptr, q_out, norm_out, false, stream, divisor,
                       avg_out, 0, &ai);
  }
  // other encoders: the decoder's accumulate, then the fused step (the same bytes)
  float* sum = acc_out ? acc_out : avg_out;
  if (sum != acc && p->n_flat > 0) {  // the tensors' elements only: sum's padding is not written
    hipLaunchKernelGGL(items_f32_kernel<false>, dim3((unsigned)p->n_flat), dim3(kThreads), 0, st, (const Item*)p->d_flat,
                       acc, sum, 1.0f);
    OMF_HIP(hipGetLastError());
  }
  if (int r = omf_qsgd_decode(p, q_in, width_in, levels_in, norm_in, sum, 1, stream)) return r;
  return omf_ps_apply_encode(p, sum, divisor, avg_out, bit_width, u, seed, offset, q_out, norm_out, stream);
}

int omf_qsgd_norms(omf_plan* plan, const float* x, float alpha, float* norm_out, void* stream) {
  return encode_impl(plan, x, alpha, 0, nullptr, 0, 0, nullptr, nullptr, norm_out, true, stream);
}

}  // extern "C"

