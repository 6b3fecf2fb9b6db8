// omf_qsgd_enc.h — device steps shared by the QSGD encoders of omf_qsgd.hip and omf_qsgd_bracket.hip
// (gfx950).
//
// The element math is omf_qsgd_dev.h; here is what the encoder kernels build on it: their argument
// record, the tail-safe quad load and payload store, a thread's row loads with their scale and sum of
// squares, the Philox draws of a row group, the quantise-and-store of a sub-chunk.  Every function is
// __device__ __forceinline__ in an unnamed namespace, as the kernels are: each unit compiles its own
// copy, and a kernel's name keeps its argument type.
#pragma once

#include "omf_common.h"
#include "omf_plan_layout.h"
#include "omf_qsgd_dev.h"

namespace {

using namespace omf;
using namespace omf::plan_layout;  // Item, TensorInfo

struct EncArgs {
  const float* x;
  const float* u;
  const float* norm_in;
  void* q;
  float* norm_out;
  const Item* items;
  const TensorInfo* tinfo;
  uint64_t* partials;  // fp64 bit patterns
  uint32_t* ticket;
  uint32_t* err;
  uint32_t* counters;
  uint64_t* gran;
  float alpha;
  uint32_t fmt;  // value format (omf_qsgd_dev.h kFmt*)
  float levels;  // 2^s as float (exact)
  uint32_t seed_lo, seed_hi, offset;
  uint64_t wait_ticks;  // bounded norm wait (100 MHz ticks)
  uint32_t epoch;       // per-launch granule tag (never 0)
  uint32_t n_items;     // items of this launch (the last ticket resets the counter)
};

// ---------------------------------------------------------------- tail-safe quads
// A quad at element e of a range that ends at `end`: whole (one 16-byte access), else its up to three
// elements one by one (absent ones read 0).  FULL: the caller knows that it is whole (no bounds checks).
// NT: a last read (the second pass of a two-pass tensor, the bracketed pass).
template <bool FULL, bool NT = false>
__device__ __forceinline__ float4 load_quad(const float* p, int64_t e, int64_t end) {
  if (FULL || e + 4 <= end) {
    if (NT) {
      const f32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p + e));
      return make_float4(t[0], t[1], t[2], t[3]);
    }
    return *reinterpret_cast<const float4*>(p + e);
  }
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < end) t.x = p[e];
  if (e + 1 < end) t.y = p[e + 1];
  if (e + 2 < end) t.z = p[e + 2];
  return t;
}

// The payload's quad (WIDTH 1: int8, 4: int32) of a live quad (e < end); non-temporal when whole.
template <int WIDTH, bool FULL = false>
__device__ __forceinline__ void store_quad(const EncArgs& a, int64_t e, int64_t end, const int32_t (&qq)[4]) {
  if (WIDTH == 1) {
    int8_t* q8 = reinterpret_cast<int8_t*>(a.q);
    if (FULL || e + 4 <= end) {
      store_nt(reinterpret_cast<uint32_t*>(q8 + e), pack_i8x4(qq));
    } else {
      q8[e] = (int8_t)qq[0];
      if (e + 1 < end) q8[e + 1] = (int8_t)qq[1];
      if (e + 2 < end) q8[e + 2] = (int8_t)qq[2];
    }
  } else {
    int32_t* q32 = reinterpret_cast<int32_t*>(a.q);
    if (FULL || e + 4 <= end) {
      store_nt(q32 + e, make_int4(qq[0], qq[1], qq[2], qq[3]));
    } else {
      q32[e] = qq[0];
      if (e + 1 < end) q32[e + 1] = qq[1];
      if (e + 2 < end) q32[e + 2] = qq[2];
    }
  }
}

// ---------------------------------------------------------------- a thread's rows
// Row k of thread tid in a sub-chunk starting at b is the quad at b + 4 (k kThreads + tid).

template <int V, bool FULL, bool NT = false>
__device__ __forceinline__ void load_f4(const float* __restrict__ p, int64_t b, int64_t end, float4 (&v)[V],
                                        int tid) {
#pragma unroll
  for (int k = 0; k < V; ++k) v[k] = load_quad<FULL, NT>(p, b + 4 * ((int64_t)k * kThreads + tid), end);
}
template <int V, bool FULL, bool NT = false>
__device__ __forceinline__ void load_f4(const float* __restrict__ p, int64_t b, int64_t end, float4 (&v)[V]) {
  load_f4<V, FULL, NT>(p, b, end, v, (int)threadIdx.x);
}

// The quad's four products with alpha.
__device__ __forceinline__ float4 mul4(float4 v, float alpha) {
  v.x = __fmul_rn(v.x, alpha); v.y = __fmul_rn(v.y, alpha);
  v.z = __fmul_rn(v.z, alpha); v.w = __fmul_rn(v.w, alpha);
  return v;
}
// x * alpha (the client weighting), rounded to the value format for bf16/fp16 tensors
// (torch.mul on a reduced-precision tensor rounds its product; with alpha = 1 it is exact).
template <int V, class A>
__device__ __forceinline__ void scale_f4(float4 (&v)[V], const A& a) {
  const float alpha = a.alpha;
  if (alpha == 1.0f) return;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    v[k] = mul4(v[k], alpha);
    if (a.fmt) v[k] = round_fmt4(v[k], a.fmt);
  }
}

// s + the quad's sum of squares: one fp32 fma chain.
__device__ __forceinline__ float sq4(float4 v, float s) {
  s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s);
  s = fmaf(v.z, v.z, s); return fmaf(v.w, v.w, s);
}
template <int V>
__device__ __forceinline__ float sumsq_f4(const float4 (&v)[V], float acc) {
#pragma unroll
  for (int k = 0; k < V; ++k) acc = sq4(v[k], acc);
  return acc;
}

// ---------------------------------------------------------------- draws

// Uniforms of rows k = 4g .. 4g+3 of this thread in a sub-chunk starting at b (the tensor begins at
// tbegin): 3 Philox calls per 16 elements (oracle/philox.py: group G, 96-bit slots).
__device__ __forceinline__ void philox_rows(const EncArgs& a, int64_t b, int64_t tbegin, int32_t tensor, int g,
                                            float4 (&uu)[4], int tid) {
  const uint64_t G = ((uint64_t)((b - tbegin) >> 12) + (uint64_t)g) * (uint64_t)kThreads + (uint32_t)tid;
  uint32_t w[12];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint64_t ctr = 3 * G + c;
    const uint4 r = philox4x32_10(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)tensor, a.offset),
                                  a.seed_lo, a.seed_hi);
    w[4 * c] = r.x; w[4 * c + 1] = r.y; w[4 * c + 2] = r.z; w[4 * c + 3] = r.w;
  }
#pragma unroll
  for (int sl = 0; sl < 4; ++sl) uu[sl] = u24x4(w[3 * sl], w[3 * sl + 1], w[3 * sl + 2]);
}
__device__ __forceinline__ void philox_rows(const EncArgs& a, int64_t b, int64_t tbegin, int32_t tensor, int g,
                                            float4 (&uu)[4]) {
  philox_rows(a, b, tbegin, tensor, g, uu, (int)threadIdx.x);
}

// ---------------------------------------------------------------- quantise and store

// Quantise V float4 of one sub-chunk starting at b (tensor t begins at tbegin) and store.
// FULL: the sub-chunk is complete (no bounds checks).
template <int WIDTH, bool HAS_U, bool FULL, int V>
__device__ __forceinline__ void quant_store(const float4 (&v)[V], const EncArgs& a, int64_t b, int64_t end,
                                            int64_t tbegin, int32_t tensor, float norm) {
  static_assert(V % 4 == 0, "rows come in groups of 4 (RNG slots)");
  const bool zero = !(norm != 0.0f);  // norm == 0: all-zero payload (reference: dense passthrough)
  const Divisor dv(norm, a.fmt);
#pragma unroll
  for (int g = 0; g < V / 4; ++g) {
    float4 uu[4];
    if (HAS_U) {
#pragma unroll
      for (int sl = 0; sl < 4; ++sl)
        uu[sl] = load_quad<FULL>(a.u, b + 4 * ((int64_t)(4 * g + sl) * kThreads + threadIdx.x), end);
    } else {
#ifdef OMF_EXP_NORNG  // experiment builds only: price the RNG
      for (int sl = 0; sl < 4; ++sl) uu[sl] = make_float4(0.5f, 0.25f, 0.75f, 0.125f);
#else
      philox_rows(a, b, tbegin, tensor, g, uu);
#endif
    }
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      const int k = 4 * g + sl;
      const int64_t e = b + 4 * ((int64_t)k * kThreads + threadIdx.x);
      if (!FULL && e >= end) continue;
      int32_t qq[4];
      qsgd_quad(v[k], uu[sl], dv, a.levels, zero, qq);
      store_quad<WIDTH, FULL>(a, e, end, qq);
    }
  }
}

// Load + scale + quantise + store one sub-chunk [b, e) of V rows (V * 1024 elements).
template <int WIDTH, bool HAS_U, int V, bool NT = false>
__device__ __forceinline__ void quant_sub(const EncArgs& a, int64_t b, int64_t e, int64_t tbegin, int32_t tensor,
                                          float norm) {
  float4 v[V];
  if (e - b == (int64_t)V * 1024) {
    load_f4<V, true, NT>(a.x, b, e, v);
    scale_f4<V>(v, a);
    quant_store<WIDTH, HAS_U, true, V>(v, a, b, e, tbegin, tensor, norm);
  } else {
    load_f4<V, false, NT>(a.x, b, e, v);
    scale_f4<V>(v, a);
    quant_store<WIDTH, HAS_U, false, V>(v, a, b, e, tbegin, tensor, norm);
  }
}

}  // namespace
