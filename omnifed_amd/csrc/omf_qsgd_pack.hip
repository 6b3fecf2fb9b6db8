// omf_qsgd_pack.hip — opt-in bit-packed QSGD wire format, MI355X (gfx950).
//
// NOT reference-compatible: a new compression_type ("QSGDBitPackedCompression") that a
// sender uses only when asked to.  The levels q in [-L, L] of the reference wire (int8 or
// int32 per element, global_grpc_compression.py:111-123) become the codes q + L in
// b = ceil(log2(2L + 1)) bits (s = 4: 6 bits instead of 8; s = 8: 10 instead of 32),
// LSB-first little-endian: element i of a tensor occupies bits [i*b, (i+1)*b) of the
// tensor's stream.  In a plan's packed arena, tensor t's stream starts at 32-bit word
// offset_t * b / 32 (the offsets must be multiples of 32 elements, else OMF_EINVAL;
// arena_layout's are multiples of 64), so 32 consecutive elements are exactly b words, lie in
// one tensor, and one thread packs or unpacks them alone.
// Decoding the codes gives the same floats as decoding the levels: both wires decode an element with
// qsgd_dec_elem and chain the sums' groups by sum_group (omf_qsgd_dec.h).
#include <cstdint>

#include "../../include/omf_codec.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_dec.h"

using namespace omf;

namespace {

constexpr int64_t kTableBlk = omf::plan_layout::kDecBlk;  // elements per decoder-table block
constexpr int kGroupBlk = 32 * kThreads;  // elements per workgroup of the pack and the decode
static_assert(kGroupBlk == 2 * kTableBlk, "two table blocks per workgroup");

// A thread's 32-element group: the whole workgroup inside one tensor (both table blocks marked
// inside the same tensor), or the group's own tensor found from the block's first one (offsets
// are multiples of 32: a group never spans two tensors).  Returns the elements of the group in
// its tensor (0 = padding, the gap in front of the first tensor included, or past the arena) and
// that tensor.
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

// Pack over the arena, one workgroup per 8 Ki-element block: each thread packs its 32-element
// group into b words.  The payload loads are issued before the block's table entry arrives,
// clamped to the last whole group of the arena (a thread whose group is whole in its tensor
// reads exactly its own elements); a group a tensor ends inside reloads its elements one by
// one and packs code 0 after them; padding groups are not written.
// B: compile-time code width (2..10, s = 0..8), or 0 = the runtime width b.
template <int WIDTH, int B>
__global__ __launch_bounds__(kThreads) void qsgd_pack(const void* __restrict__ q, const uint32_t* __restrict__ binfo,
                                                      int64_t nbinfo, const int64_t* __restrict__ begins,
                                                      const int64_t* __restrict__ sizes, int32_t nt, int64_t arena_end,
                                                      int32_t L, int32_t b_rt, uint32_t* __restrict__ out) {
  const int b = B ? B : b_rt;
  const int64_t e0 = (int64_t)blockIdx.x * kGroupBlk + 32 * (int64_t)threadIdx.x;
  const int64_t qmax = ((arena_end >> 5) - 1) << 5;  // the last whole group (< 0: none)
  const int64_t ec = max((int64_t)0, min(e0, qmax));
  int32_t lv[32];
  if (qmax >= 0) {  // uniform
    if (WIDTH == 1) {
      const int8_t* q8 = static_cast<const int8_t*>(q) + ec;
      const i32x4_t w0 = *reinterpret_cast<const i32x4_t*>(q8);
      const i32x4_t w1 = *reinterpret_cast<const i32x4_t*>(q8 + 16);
      const uint32_t w[8] = {(uint32_t)w0[0], (uint32_t)w0[1], (uint32_t)w0[2], (uint32_t)w0[3],
                             (uint32_t)w1[0], (uint32_t)w1[1], (uint32_t)w1[2], (uint32_t)w1[3]};
#pragma unroll
      for (int i = 0; i < 32; ++i) lv[i] = (int32_t)(int8_t)(w[i >> 2] >> (8 * (i & 3)));
    } else {
      const int32_t* q32 = static_cast<const int32_t*>(q) + ec;
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const i32x4_t w = *reinterpret_cast<const i32x4_t*>(q32 + 4 * v);
        lv[4 * v] = w[0]; lv[4 * v + 1] = w[1]; lv[4 * v + 2] = w[2]; lv[4 * v + 3] = w[3];
      }
    }
  }
  bool whole;
  int32_t t;
  const int nv = group_tensor(binfo, nbinfo, begins, sizes, nt, e0, &whole, &t);
  if (nv == 0) return;
  if (nv < 32) {  // the tensor ends inside this group (its elements only; codes 0 after them)
#pragma unroll
    for (int i = 0; i < 32; ++i)
      lv[i] = i < nv ? (WIDTH == 1 ? (int32_t)(static_cast<const int8_t*>(q)[e0 + i])
                                   : static_cast<const int32_t*>(q)[e0 + i])
                     : -L;
  }
  uint32_t* o = out + (e0 >> 5) * (int64_t)b;
  uint32_t wd[B ? B : 32];
  uint64_t acc = 0;
  int nb = 0, w = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    acc |= (uint64_t)((uint32_t)lv[i] + (uint32_t)L) << nb;  // modulo 2^32: q + L passes INT32_MAX from L = 2^30 on
    nb += b;
    if (nb >= 32) {
      if (B) wd[w++] = (uint32_t)acc;  // static index once unrolled
      else o[w++] = (uint32_t)acc;     // runtime width: straight to memory
      acc >>= 32;
      nb -= 32;
    }
  }
  if (B && B % 2 == 0) {  // b words at a multiple of 8 bytes: 8-byte stores
#pragma unroll
    for (int i = 0; i < (B ? B : 2); i += 2)
      *reinterpret_cast<uint2*>(o + i) = make_uint2(wd[i], wd[i + 1]);
  } else if (B) {
#pragma unroll
    for (int i = 0; i < (B ? B : 1); ++i) o[i] = wd[i];
  }
}

// Decode over the arena, one workgroup per 8 Ki-element block (two blocks of the plan's 4 Ki
// decoder table, omf_qsgd_recv.hip qsgd_decode_arena): every lane's b packed words go out first, their
// addresses depending on blockIdx only, with the block's tensor and norm as scalar loads in
// flight (the item-indexed version waited for its item and norm, then walked its item pass by
// pass: 0.38 ms on Llama-400M).  Each thread unpacks its 32 elements into LDS; the workgroup
// transposes them (33-word rows: conflict-free both ways) so the fp32 stores are lane-contiguous
// 16-byte non-temporal stores.  A block not inside one tensor finds each 32-element group's
// tensor (packed_arena requires offsets that are multiples of 32: a group never spans two) and
// writes only its elements;
// padding keeps what y held.
template <int B, bool ACC, bool POW2>
__global__ __launch_bounds__(kThreads) void qsgd_decode_packed(const uint32_t* __restrict__ packed,
                                                               const uint32_t* __restrict__ binfo, int64_t nbinfo,
                                                               const float* __restrict__ norm,
                                                               const int64_t* __restrict__ begins,
                                                               const int64_t* __restrict__ sizes, int32_t nt,
                                                               int64_t arena_end, float* __restrict__ y, int32_t L,
                                                               int32_t b_rt, float levels, float inv_levels) {
  constexpr int G = kGroupBlk;
  __shared__ float tile[kThreads * 33];
  __shared__ int32_t s_lim[kThreads];
  const int b = B ? B : b_rt;
  const int64_t base = (int64_t)blockIdx.x * G;
  const int64_t e0 = base + 32 * (int64_t)threadIdx.x;
  // unconditional loads, clamped to the packed arena's last group
  const uint32_t* p = packed + min(e0 >> 5, (arena_end - 1) >> 5) * (int64_t)b;
  uint32_t wd[B ? B : 32];
  if (B) {
#pragma unroll
    for (int i = 0; i < (B ? B : 1); ++i) wd[i] = __builtin_nontemporal_load(p + i);
  } else {
    for (int i = 0; i < b; ++i) wd[i] = p[i];
  }
  bool whole;
  int32_t t;
  const int lim = group_tensor(binfo, nbinfo, begins, sizes, nt, e0, &whole, &t);
  if (!whole) s_lim[threadIdx.x] = lim;
  const float nrm = lim > 0 ? norm[t] : 0.0f;
  const uint64_t mask = (1ull << b) - 1ull;
  uint64_t acc = 0;
  int nb = 0, w = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    if (nb < b) {
      acc |= (uint64_t)wd[w++] << nb;
      nb += 32;
    }
    const int32_t qi = (int32_t)((uint32_t)(acc & mask) - (uint32_t)L);  // modulo 2^32 (b = 32: codes above INT32_MAX)
    acc >>= b;
    nb -= b;
    tile[threadIdx.x * 33 + i] = qsgd_dec_elem<POW2>(nrm, qi, levels, inv_levels);
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const int e = 4 * (v * kThreads + (int)threadIdx.x);  // element of this block
    float f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = tile[((e + c) >> 5) * 33 + ((e + c) & 31)];
    float* yo = y + base + e;
    const int l = whole ? 4 : s_lim[e >> 5] - (e & 31);  // elements of the quad to write
    if (l >= 4) {
      float4 o = make_float4(f[0], f[1], f[2], f[3]);
      if (ACC) {
        const f32x4_t pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(yo));
        o.x = __fadd_rn(pv[0], o.x); o.y = __fadd_rn(pv[1], o.y);
        o.z = __fadd_rn(pv[2], o.z); o.w = __fadd_rn(pv[3], o.w);
      }
      store_nt(yo, o);
    } else {
      for (int c = 0; c < l; ++c) yo[c] = ACC ? __fadd_rn(yo[c], f[c]) : f[c];
    }
  }
}

// N clients' packed payloads decoded and summed in one pass (omf_qsgd_decode_sum_packed), in
// qsgd_decode_packed's shape: one workgroup per 8 Ki-element block, one 32-element group per thread.
//   s = init ? y : +0;  s = fl32(s + qsgd_dec_elem(norm_c[t], code_c - L))  c = 0..N-1;
//   y = divisor != 0 ? s / divisor : s
// the bytes of omf_qsgd_decode_sum on the same levels unpacked.  All N clients' b words of the
// thread's group go out first (unconditional, clamped to the packed arena's last group), with the
// block's table entry and the N norms in flight; the 32 running sums stay in registers, added in
// client order.  With `init` the sums start from y, which is read as lane-contiguous 16-byte loads
// and brought into group order through the 33-word-row tile (fp32 addition does not let y be added
// last); the sums leave through the same tile as lane-contiguous non-temporal 16-byte stores.
// The client pointers are kernel arguments indexed at compile time (N is a template parameter: a
// runtime index into a by-value array is copied to scratch).  A block not inside one tensor finds
// each group's tensor and goes element by element where a tensor ends inside a quad; with `fill`
// it also writes the padding of [0, arena_end) (fl32(+0 / pad_div), or +0), otherwise padding is
// neither read nor written.
// B: compile-time code width (2..10), or 0 = the runtime width b_rt, whose codes are read from
// memory element by element (a register array indexed by a runtime word count goes to scratch).
constexpr int kPackedSumMax = 8;     // clients per launch; omf_qsgd_decode_sum_packed chains groups
constexpr int kPackedSumMaxWide = 4; // the same for the runtime-width instance (32 * N unrolled two-word reads)
template <int N>
struct PackedSumArgs {
  const uint32_t* packed[N];
  const float* norm[N];
  float* y;
  float levels;      // fl32(levels)
  float inv_levels;  // 1 / levels for a power of two (exact), else unused
  float divisor;     // 0: no division
  float pad_div;     // the whole call's divisor: what the padding is divided by (fill)
  int32_t init;      // the sum starts from y (else from +0: y is not read)
  int32_t fill;      // padding elements of [0, arena_end) are written
  int32_t L;
  int32_t b_rt;
};

template <int B, bool POW2, int N>
__global__ __launch_bounds__(kThreads) void qsgd_decode_sum_packed(PackedSumArgs<N> a,
                                                                   const uint32_t* __restrict__ binfo, int64_t nbinfo,
                                                                   const int64_t* __restrict__ begins,
                                                                   const int64_t* __restrict__ sizes, int32_t nt,
                                                                   int64_t arena_end) {
  constexpr int G = kGroupBlk;
  __shared__ float tile[kThreads * 33];
  __shared__ int32_t s_lim[kThreads];
  const int b = B ? B : a.b_rt;
  const int64_t base = (int64_t)blockIdx.x * G;
  const int64_t e0 = base + 32 * (int64_t)threadIdx.x;
  // unconditional loads, clamped to the packed arena's last group
  const int64_t woff = min(e0 >> 5, (arena_end - 1) >> 5) * (int64_t)b;
  uint32_t wd[N][B ? B : 1];
  if (B) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
#pragma unroll
      for (int i = 0; i < (B ? B : 1); ++i) wd[c][i] = __builtin_nontemporal_load(a.packed[c] + woff + i);
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
  for (int c = 0; c < N; ++c) nrm[c] = lim > 0 ? a.norm[c][t] : 0.0f;
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
    const uint32_t* p = a.packed[c] + woff;
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
      const int32_t qi = (int32_t)(code - (uint32_t)a.L);
      s[i] = __fadd_rn(s[i], qsgd_dec_elem<POW2>(nrm[c], qi, a.levels, a.inv_levels));
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

// The plan's arena as the pack and the decode walk it.
struct ArenaArgs {
  const uint32_t* binfo;
  int64_t nbinfo;
  const int64_t* begins;
  const int64_t* sizes;
  int32_t nt;
  int64_t arena_end;
};

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

template <int WIDTH>
void dispatch_pack(int b, dim3 g, hipStream_t st, const void* q, const ArenaArgs& a, int32_t L, uint32_t* out) {
  with_code_bits(b, [&](auto B) {
    hipLaunchKernelGGL((qsgd_pack<WIDTH, B()>), g, dim3(kThreads), 0, st, q, a.binfo, a.nbinfo, a.begins, a.sizes, a.nt,
                       a.arena_end, L, b, out);
  });
}

template <bool ACC, bool POW2>
void dispatch_decode(int b, dim3 g, hipStream_t st, const uint32_t* packed, const ArenaArgs& a, const float* norm,
                     float* y, int32_t L, float levels, float inv) {
  with_code_bits(b, [&](auto B) {
    hipLaunchKernelGGL((qsgd_decode_packed<B(), ACC, POW2>), g, dim3(kThreads), 0, st, packed, a.binfo, a.nbinfo, norm,
                       a.begins, a.sizes, a.nt, a.arena_end, y, L, b, levels, inv);
  });
}

// ---- omf_qsgd_decode_sum_packed: one group of at most kPackedSumMax clients per launch
struct PackedSumCall : SumCallBase {
  ArenaArgs a;
  dim3 grid;
  const uint32_t* const* packed;
  int32_t L, b;
};

template <int B, bool P, int N>
void launch_psum_n(const PackedSumCall& c) {
  PackedSumArgs<N> k{};
  for (int i = 0; i < N; ++i) k.packed[i] = c.packed[i];
  sum_common_args(k, c, N);
  k.L = c.L; k.b_rt = c.b;
  hipLaunchKernelGGL((qsgd_decode_sum_packed<B, P, N>), c.grid, dim3(kThreads), 0, c.st, k, c.a.binfo, c.a.nbinfo,
                     c.a.begins, c.a.sizes, c.a.nt, c.a.arena_end);
}

template <bool P>
void dispatch_psum(const PackedSumCall& c, int n) {
  with_code_bits(c.b, [&](auto B) {
    with_group_size<(B() != 0 ? kPackedSumMax : kPackedSumMaxWide)>(n, [&](auto N) { launch_psum_n<B(), P, N()>(c); });
  });
}

// The plan's arena for the packed wire, or an error: every tensor offset a multiple of 32
// elements (a tensor's stream then starts on a word, and a 32-element group lies in one tensor).
int packed_arena(const omf_plan* plan, ArenaArgs* a, dim3* grid) {
  for (const int64_t o : plan->offsets)
    if (o & 31) return fail(OMF_EINVAL, "the packed wire needs tensor offsets that are multiples of 32 elements");
  a->binfo = plan->d_dec_binfo;
  a->nbinfo = plan->n_dec_blocks;
  a->begins = plan->d_begins;
  a->sizes = plan->d_sizes;
  a->nt = plan->nt;
  a->arena_end = plan->arena_end;
  *grid = dim3((unsigned)((a->arena_end + kGroupBlk - 1) / kGroupBlk));
  return OMF_OK;
}

}  // namespace

extern "C" {

int32_t omf_qsgd_packed_bits(int32_t levels) {
  if (levels <= 0 || levels == INT32_MAX) return -1;  // the wire's levels: [1, 2^31 - 1), as the binding's
  const uint64_t codes = 2ull * (uint64_t)levels + 1ull;
  int32_t b = 0;
  while ((1ull << b) < codes) ++b;
  return b;
}

int omf_qsgd_pack(omf_plan* plan, const void* q, int32_t width, int32_t levels, uint32_t* packed, void* stream) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (width != 8 && width != 32) return fail(OMF_EINVAL, "width must be 8 or 32");
  const int32_t b = omf_qsgd_packed_bits(levels);
  if (b < 0 || b > 32) return fail(OMF_EINVAL, "levels must be in [1, 2^31 - 1)");
  if (width == 8 && levels > 127) return fail(OMF_EINVAL, "an int8 payload holds levels <= 127");
  if (!q || !packed) return fail(OMF_EINVAL, "q and packed must be non-NULL");
  // even widths store 8-byte word pairs: the packed arena must be 8-byte aligned
  if (!aligned(q, 16) || !aligned(packed, 8)) return fail(OMF_EINVAL, "q must be 16-byte, packed 8-byte aligned");
  ArenaArgs a;
  dim3 grid;
  if (const int rc = packed_arena(plan, &a, &grid)) return rc;
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  if (width == 8) dispatch_pack<1>(b, grid, st, q, a, levels, packed);
  else dispatch_pack<4>(b, grid, st, q, a, levels, packed);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf_qsgd_decode_packed(omf_plan* plan, const uint32_t* packed, int32_t levels, const float* norm, float* y,
                           int32_t accumulate, void* stream) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  const int32_t b = omf_qsgd_packed_bits(levels);
  if (b < 0 || b > 32) return fail(OMF_EINVAL, "levels must be in [1, 2^31 - 1)");
  if (!packed || !norm || !y) return fail(OMF_EINVAL, "packed, norm and y must be non-NULL");
  if (!aligned(y, 16) || !aligned(packed, 4)) return fail(OMF_EINVAL, "y must be 16-byte, packed 4-byte aligned");
  ArenaArgs a;
  dim3 grid;
  if (const int rc = packed_arena(plan, &a, &grid)) return rc;
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  const LevelScale lv(levels);
#define OMF_DD(A, P) dispatch_decode<A, P>(b, grid, st, packed, a, norm, y, levels, lv.levels, lv.inv_levels)
  if (accumulate) {
    if (lv.pow2) OMF_DD(true, true); else OMF_DD(true, false);
  } else {
    if (lv.pow2) OMF_DD(false, true); else OMF_DD(false, false);
  }
#undef OMF_DD
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf_qsgd_decode_sum_packed(omf_plan* plan, const uint32_t* const* packed, const float* const* norm,
                               int32_t nclients, int32_t levels, float* y, int32_t init, float divisor, void* stream) {
  if (nclients < 1) return fail(OMF_EINVAL, "omf_qsgd_decode_sum_packed: nclients must be >= 1");
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  const int32_t b = omf_qsgd_packed_bits(levels);
  if (b < 0 || b > 32) return fail(OMF_EINVAL, "levels must be in [1, 2^31 - 1)");
  if (!packed || !norm || !y) return fail(OMF_EINVAL, "packed, norm and y_out must be non-NULL");
  if (!aligned(y, 16)) return fail(OMF_EINVAL, "y_out must be 16-byte aligned");
  PackedSumCall c;
  if (const int rc = packed_arena(plan, &c.a, &c.grid)) return rc;
  const size_t ybytes = (size_t)plan->arena_end * 4;
  const size_t pbytes = (size_t)((plan->arena_end + 31) / 32) * (size_t)b * 4;
  for (int32_t k = 0; k < nclients; ++k) {
    if (!packed[k] || !norm[k]) return fail(OMF_EINVAL, "omf_qsgd_decode_sum_packed: a NULL entry in packed or norm");
    if (!aligned(packed[k], 4)) return fail(OMF_EINVAL, "a packed arena must be 4-byte aligned");
    if (overlaps(y, ybytes, packed[k], pbytes) || overlaps(y, ybytes, norm[k], (size_t)plan->nt * 4))
      return fail(OMF_EINVAL, "omf_qsgd_decode_sum_packed: y_out overlaps a packed or norm buffer");
  }
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const LevelScale lv(levels);
  c.y = y; c.st = (hipStream_t)stream; c.L = levels; c.b = b; c.levels = lv.levels; c.inv_levels = lv.inv_levels;
  const int32_t per = b <= 10 ? kPackedSumMax : kPackedSumMaxWide;
  for (int32_t k0 = 0; k0 < nclients; k0 += per) {  // the chained groups (sum_group, omf_qsgd_dec.h)
    c.g = sum_group(nclients, per, init, divisor, k0);
    c.packed = packed + k0; c.norm = norm + k0;
    if (lv.pow2) dispatch_psum<true>(c, c.g.n); else dispatch_psum<false>(c, c.g.n);
    OMF_HIP(hipGetLastError());
  }
  return OMF_OK;
}

}  // extern "C"
