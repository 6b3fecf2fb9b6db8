// omf_qsgd_dec.h — the QSGD receive side's rules, one copy of each: shared by omf_qsgd_recv.hip (the int8 /
// int32 wire) and omf_qsgd_pack.hip (the bit-packed wire); omf_qsgd.hip and omf_qsgd_bracket.hip take the
// pointer checks and the element decode from it.  Not part of the C ABI.  The host rules come first and are
// plain C++ with no HIP header (tests/host/qsgd_dec_check.cpp builds them with g++ and the sanitizers); the
// device rules and the sum calls' shared record follow under __HIPCC__.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace omf {

// ---------------------------------------------------------------- host rules

// fl32(levels) and, for a power of two, the exact 2^-s a decoder multiplies by in place of the division
// (else 0, unused).  levels > 0.
struct LevelScale {
  float levels, inv_levels;
  bool pow2;
  explicit LevelScale(int32_t l) : levels((float)l), inv_levels(0.0f), pow2((l & (l - 1)) == 0) {
    if (pow2) inv_levels = 1.0f / levels;
  }
};

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// [a, a + na) and [b, b + nb) share a byte (an empty range shares none; the callers' ranges never are).
inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// One launch of a sum over `nclients` payloads, chained in groups of at most `per` clients in order.
struct SumGroup {
  int32_t n;      // clients k0 .. k0 + n - 1
  int32_t init;   // the sum starts from y (else from +0: y is not read)
  int32_t fill;   // padding elements of [0, arena_end) are written
  float divisor;  // 0: no division
  float pad_div;  // the whole call's divisor: what the padding is divided by (fill)
};

// The group that starts at client k0 (k0 = 0, per, 2 per, ... < nclients): every group but the first
// starts from y, the first fills the padding unless the call's `init`, only the last divides.
inline SumGroup sum_group(int32_t nclients, int32_t per, int32_t init, float divisor, int32_t k0) {
  SumGroup g;
  g.n = nclients - k0 < per ? nclients - k0 : per;
  g.init = (k0 > 0 || init) ? 1 : 0;
  g.fill = (k0 == 0 && !init) ? 1 : 0;
  g.divisor = k0 + g.n == nclients ? divisor : 0.0f;
  g.pad_div = divisor;
  return g;
}

// f(std::integral_constant<int, n>) for a group of n = 1 .. MAX clients: the sum kernels take the group's
// size at compile time.
template <int MAX, class F>
void with_group_size(int n, F&& f) {
  if constexpr (MAX > 1) {
    if (n < MAX) return with_group_size<MAX - 1>(n, f);
  }
  f(std::integral_constant<int, MAX>{});
}

}  // namespace omf

#ifdef __HIPCC__
#include "omf_common.h"

namespace omf {

// What a sum launch takes from its call on either wire; SumArgs<N> and PackedSumArgs<N> hold the same
// fields under the same names.
struct SumCallBase {
  const float* const* norm;
  float* y;
  float levels, inv_levels;
  SumGroup g;
  hipStream_t st;
};

template <class Args>
void sum_common_args(Args& a, const SumCallBase& c, int n) {
  for (int k = 0; k < n; ++k) a.norm[k] = c.norm[k];
  a.y = c.y; a.levels = c.levels; a.inv_levels = c.inv_levels; a.divisor = c.g.divisor; a.pad_div = c.g.pad_div;
  a.init = c.g.init; a.fill = c.g.fill;
}

// ---------------------------------------------------------------- device rules

// One element: fl32(fl32(norm * q) / levels).  (norm * q) / 2^s == (norm * q) * 2^-s exactly (power-of-two
// scaling, both correctly rounded), so POW2 multiplies by inv_levels.
template <bool POW2>
__device__ __forceinline__ float qsgd_dec_elem(float norm, int32_t q, float levels, float inv_levels) {
  const float nq = __fmul_rn(norm, (float)q);
  return POW2 ? __fmul_rn(nq, inv_levels) : nq / levels;
}

// The four sign-extended int8 levels of a payload dword.
__device__ __forceinline__ void qsgd_split_i8(int32_t w, int32_t (&qi)[4]) {
  qi[0] = (int32_t)(int8_t)(w & 0xff);
  qi[1] = (int32_t)(int8_t)((w >> 8) & 0xff);
  qi[2] = (int32_t)(int8_t)((w >> 16) & 0xff);
  qi[3] = (int32_t)(int8_t)((w >> 24) & 0xff);
}

// A tensor's partial last quad at element e (the tensor ends at te, e + 4 > te): its bytes (WIDTH 1, in
// rr[0]) or dwords only — at most three elements read, zeros after them — since the payload may end here.
template <int WIDTH>
__device__ __forceinline__ void qsgd_last_quad(const void* q, int64_t e, int64_t te, int32_t (&rr)[4]) {
  if (WIDTH == 1) {
    const int8_t* q8 = reinterpret_cast<const int8_t*>(q);
    uint32_t w = 0;
    for (int c = 0; c < 3; ++c)
      if (e + c < te) w |= (uint32_t)(uint8_t)q8[e + c] << (8 * c);
    rr[0] = (int32_t)w;
  } else {
    const int32_t* q32 = reinterpret_cast<const int32_t*>(q);
    for (int c = 0; c < 3; ++c) rr[c] = e + c < te ? q32[e + c] : 0;
    rr[3] = 0;
  }
}

// The last tensor that starts at or before element e, walking up from t0, the first tensor of e's
// decoder-table block (a boundary block: at most a few steps).
__device__ __forceinline__ int32_t qsgd_tensor_at(int32_t t0, int64_t e, const int64_t* __restrict__ begins,
                                                  int32_t nt) {
  int32_t t = t0;
  while (t + 1 < nt && e >= begins[t + 1]) ++t;
  return t;
}

}  // namespace omf
#endif  // __HIPCC__
