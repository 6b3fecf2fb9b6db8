// omf_qsgd_dec.h — the QSGD receive side's rules, one copy of each: shared by omf_qsgd_recv.hip (the int8 /
// int32 wire), omf_qsgd_pack.hip (the bit-packed wire) and omf_qsgd_bucket_pack.hip (bucket norms on the bit-packed
// wire: the packed rules at the end are theirs); omf_qsgd.hip and omf_qsgd_bracket.hip take the
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

// ---------------------------------------------------------------- the bit-packed wire's rules
// (omf_qsgd_pack.hip, omf_qsgd_bucket_pack.hip)

constexpr int kGroupBlk = 32 * kThreads;  // elements per workgroup of the pack and the packed decodes

// A level's code on the packed wire and back, modulo 2^32: q + L passes INT32_MAX from L = 2^30 on, and at
// b = 32 a foreign code may lie above INT32_MAX.
__device__ __forceinline__ uint32_t qsgd_code(int32_t q, int32_t L) { return (uint32_t)q + (uint32_t)L; }
__device__ __forceinline__ int32_t qsgd_level(uint32_t code, int32_t L) { return (int32_t)(code - (uint32_t)L); }

// Word w of a 32-element group's b words, from the group's bits held as `n` consecutive units of `ub` bits each
// (n ub = 32 b; a unit is a code, ub = b, or a quad's fragment of four codes, ub = 4 b <= 64): the word is bits
// [32 w, 32 w + 32) of the units' concatenation, LSB first, so it takes units floor(32 w / ub) ..
// floor((32 w + 31) / ub) — at most `span` of them (4 for the fragments of b = 2, 3, else 3; ub is 4 b or > 16).  unit(j): unit j as uint64_t, no
// bit set at or above ub.  inv_ub = 1 / ub as a float: floor((x + 0.5) inv_ub) is floor(x / ub) exactly for the
// x < 1024 and ub <= 64 met here ((x + 0.5) / ub lies at least 1 / 128 from an integer).
template <class Unit>
__device__ __forceinline__ uint32_t group_word(int w, int ub, float inv_ub, int n, int span, Unit unit) {
  const int bit0 = 32 * w;
  const int j0 = (int)(((float)bit0 + 0.5f) * inv_ub);
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = j0 + i;
    const int sh = j * ub - bit0;  // where unit j starts in the word (negative: before it)
    if (i < span && j < n && sh < 32) {
      const uint64_t f = unit(j);
      word |= sh >= 0 ? (uint32_t)(f << sh) : (uint32_t)(f >> -sh);
    }
  }
  return word;
}

// The mirror image of group_word: the four codes of quad f (elements 4 f .. 4 f + 3, f = 0 .. 7) of a 32-element
// group from the group's b words, b <= 16.  The quad's fragment is bits [4 b f, 4 b (f + 1)) of the words'
// concatenation: it starts inside word w0 = floor(4 b f / 32) at bit sh (a multiple of 4) and ends before bit
// sh + 64 <= 92, so it lies in words w0 .. w0 + 2; every code (b <= 16 bits) is read through one 64-bit window,
// the one over words w0, w0 + 1 where it starts below bit 32 and the one over w0 + 1, w0 + 2 otherwise.  A
// window's word past the group's last (index clamped to b - 1) holds no bit of the fragment.  word(i): word i of
// the group.
template <class Word>
__device__ __forceinline__ void group_quad(int f, int b, Word word, uint32_t (&code)[4]) {
  const int bit0 = 4 * b * f, w0 = bit0 >> 5, sh = bit0 & 31;
  const uint32_t x0 = word(w0), x1 = word(min(w0 + 1, b - 1)), x2 = word(min(w0 + 2, b - 1));
  const uint64_t lo = (uint64_t)x0 | ((uint64_t)x1 << 32), hi = (uint64_t)x1 | ((uint64_t)x2 << 32);
  const uint32_t mask = (1u << b) - 1u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = sh + j * b;  // < 28 + 3 * 16 + 1
    code[j] = (uint32_t)(p < 32 ? lo >> p : hi >> (p - 32)) & mask;
  }
}

// A thread's 32-element group at e0 in a workgroup of kGroupBlk elements (two blocks of the plan's decoder
// table): the whole workgroup inside one tensor (both table blocks marked inside the same tensor), or the
// group's own tensor found from the block's first one (offsets are multiples of 32: a group never spans two
// tensors).  Returns the elements of the group in its tensor (0 = padding, the gap in front of the first
// tensor included, or past the arena) and that tensor.
__device__ __forceinline__ int group_tensor(const uint32_t* __restrict__ binfo, int64_t nbinfo,
                                            const int64_t* __restrict__ begins, const int64_t* __restrict__ sizes,
                                            int32_t nt, int64_t e0, bool* whole, int32_t* tensor) {
  const int64_t k0 = 2 * (int64_t)blockIdx.x;
  const uint32_t i0 = binfo[k0];
  const uint32_t i1 = k0 + 1 < nbinfo ? binfo[k0 + 1] : 0u;
  int32_t t = (int32_t)(i0 & 0x7fffffffu);  // the last tensor starting at or before the block
  *whole = (i0 >> 31) && i1 == i0;
  if (*whole) {
    *tensor = t;
    return 32;
  }
  while (t + 1 < nt && e0 >= begins[t + 1]) ++t;
  *tensor = t;
  if (e0 < begins[t]) return 0;  // padding before the first tensor
  const int64_t lim = min((int64_t)32, begins[t] + sizes[t] - e0);
  return lim > 0 ? (int)lim : 0;
}

// One workgroup's 8 Ki-element block of a K-client decode-and-sum over packed arenas, one 32-element group
// per thread; the kernels of both packed wires are this body (qsgd_decode_sum_packed, omf_qsgd_pack.hip, with a
// norm per tensor; qsgd_bucket_decode_sum_packed, omf_qsgd_bucket_pack.hip, with a norm per bucket).
//   s = init ? y : +0;  s = fl32(s + qsgd_dec_elem(norm_c, code_c - L))  c = 0..N-1;
//   y = divisor != 0 ? s / divisor : s
// All N clients' b words of the thread's group go out first (unconditional, clamped to the packed arena's
// last group), with the block's table entry and the N norms in flight; the 32 running sums stay in
// registers, added in client order.  With `init` the sums start from y, which is read as lane-contiguous
// 16-byte loads and brought into group order through the 33-word-row tile (fp32 addition does not let y be
// added last); the sums leave through the same tile as lane-contiguous non-temporal 16-byte stores.
// words(c): client c's packed arena; norm(c, lim, t, e0): its norm for the thread's group (lim elements of
// tensor t from e0; lim = 0: no element, any value).  c is a compile-time index once unrolled (N is a template
// parameter: a runtime index into a by-value array is copied to scratch).  A block not inside one tensor
// finds each group's tensor and goes element by element where a tensor ends inside a quad; with `fill` it
// also writes the padding of [0, arena_end) (fl32(+0 / pad_div), or +0), otherwise padding is neither read
// nor written.
// B: compile-time code width (2..10), or 0 = the runtime width b_rt, whose codes are read from memory element
// by element (a register array indexed by a runtime word count goes to scratch).
// tile: kThreads * 33 floats, s_lim: kThreads words of LDS.
template <int B, bool POW2, int N, class Args, class Words, class Norm>
__device__ __forceinline__ void packed_sum_block(const Args& a, int32_t L, int32_t b_rt, Words words, Norm norm,
                                                 const uint32_t* __restrict__ binfo, int64_t nbinfo,
                                                 const int64_t* __restrict__ begins,
                                                 const int64_t* __restrict__ sizes, int32_t nt, int64_t arena_end,
                                                 float* tile, int32_t* s_lim) {
  constexpr int G = kGroupBlk;
  const int b = B ? B : b_rt;
  const int64_t base = (int64_t)blockIdx.x * G;
  const int64_t e0 = base + 32 * (int64_t)threadIdx.x;
  // unconditional loads, clamped to the packed arena's last group
  const int64_t woff = min(e0 >> 5, (arena_end - 1) >> 5) * (int64_t)b;
  uint32_t wd[N][B ? B : 1];
  if (B) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
#pragma unroll
      for (int i = 0; i < (B ? B : 1); ++i) wd[c][i] = __builtin_nontemporal_load(words(c) + woff + i);
    }
  }
  bool whole;  // uniform: from the block's two table entries
  int32_t t;
  const int lim = group_tensor(binfo, nbinfo, begins, sizes, nt, e0, &whole, &t);
  if (!whole) {
    s_lim[threadIdx.x] = lim;
    __syncthreads();
  }
  float nrm[N];
#pragma unroll
  for (int c = 0; c < N; ++c) nrm[c] = norm(c, lim, t, e0);
  float s[32];
  if (a.init) {  // uniform
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int e = 4 * (v * kThreads + (int)threadIdx.x);  // element of this block
      const int l = whole ? 4 : s_lim[e >> 5] - (e & 31);   // elements of the quad inside a tensor
      const float* yi = a.y + base + e;
      f32x4_t pv = {0.0f, 0.0f, 0.0f, 0.0f};
      if (l >= 4) {
        pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(yi));
      } else {
        if (l > 0) pv[0] = yi[0];
        if (l > 1) pv[1] = yi[1];
        if (l > 2) pv[2] = yi[2];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) tile[((e + c) >> 5) * 33 + ((e + c) & 31)] = pv[c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 32; ++i) s[i] = tile[threadIdx.x * 33 + i];  // this thread's row: rewritten by it alone below
  } else {
#pragma unroll
    for (int i = 0; i < 32; ++i) s[i] = 0.0f;
  }
  const uint64_t mask = (1ull << b) - 1ull;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    uint64_t acc = 0;
    int nb = 0, w = 0;
    const uint32_t* p = words(c) + woff;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      uint32_t code;
      if (B) {
        if (nb < b) {
          acc |= (uint64_t)wd[c][w++] << nb;
          nb += 32;
        }
        code = (uint32_t)(acc & mask);
        acc >>= b;
        nb -= b;
      } else {  // bits [i b, (i + 1) b) of the group's b words: at most two words, both inside the group
        const int bit = i * b, wi = bit >> 5;
        const uint64_t two = ((uint64_t)p[min(wi + 1, b - 1)] << 32) | p[wi];
        code = (uint32_t)((two >> (bit & 31)) & mask);
      }
      s[i] = __fadd_rn(s[i], qsgd_dec_elem<POW2>(nrm[c], qsgd_level(code, L), a.levels, a.inv_levels));
    }
    // One client at a time: the sums are pinned in their registers here.  Left free, the compiler sinks
    // every client's unpack and adds to the end and holds all their codes at once (256 VGPRs, one
    // wave per SIMD at N = 8).
#pragma unroll
    for (int i = 0; i < 32; ++i) asm volatile("" : "+v"(s[i]));
  }
  if (a.divisor != 0.0f) {
#pragma unroll
    for (int i = 0; i < 32; ++i) s[i] = s[i] / a.divisor;
  }
#pragma unroll
  for (int i = 0; i < 32; ++i) tile[threadIdx.x * 33 + i] = s[i];
  __syncthreads();
  const float pad = a.pad_div != 0.0f ? 0.0f / a.pad_div : 0.0f;
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const int e = 4 * (v * kThreads + (int)threadIdx.x);
    float f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = tile[((e + c) >> 5) * 33 + ((e + c) & 31)];
    float* yo = a.y + base + e;
    const int l = whole ? 4 : s_lim[e >> 5] - (e & 31);
    if (l >= 4) {
      store_nt(yo, make_float4(f[0], f[1], f[2], f[3]));
    } else if (a.fill && base + e + 4 <= arena_end) {  // a quad with padding, all of it inside the arena
      store_nt(yo, make_float4(l > 0 ? f[0] : pad, l > 1 ? f[1] : pad, l > 2 ? f[2] : pad, pad));
    } else {
      for (int c = 0; c < 4; ++c) {
        if (c < l) yo[c] = f[c];
        else if (a.fill && base + e + c < arena_end) yo[c] = pad;
      }
    }
  }
}

// f(std::integral_constant<int, B>): B = b for the compile-time code widths 2..10, else 0 (the runtime width).
template <class F>
void with_code_bits(int b, F&& f) {
  switch (b) {
#define OMF_B(B) case B: f(std::integral_constant<int, B>{}); break;
    OMF_B(2) OMF_B(3) OMF_B(4) OMF_B(5) OMF_B(6) OMF_B(7) OMF_B(8) OMF_B(9) OMF_B(10)
#undef OMF_B
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

}  // namespace omf
#endif  // __HIPCC__
