// omf_qsgd_recv.hip — the QSGD receive side on the int8 / int32 wire, MI355X (gfx950): the decoders, the
// K-client decode-and-sum and the flat divide, with their host side.  The plan and the encoders are
// omf_qsgd.hip; the bit-packed wire's decoders omf_qsgd_pack.hip; the rules both wires decode by (one element,
// the int8 split, a partial last quad, a boundary block's tensor walk, the levels scale, the sums' chaining) omf_qsgd_dec.h.
//
// Kernel map:
//   qsgd_decode_arena      y = (norm * q) / L over the arena's 4 Ki blocks, optionally accumulated (PS);
//   qsgd_decode_flat       the same per flat item with byte loads: payloads of fewer than 4 elements.
//   qsgd_decode_sum_*      up to 8 clients' payloads decoded and summed in one pass (omf_qsgd_decode_sum).
//   div_f32_kernel         y /= d over a flat buffer (omf_div_f32).
//
// HBM-bound; no MFMA.  4 B/lane int8 and 16 B/lane int32 payload loads, non-temporal 16 B/lane fp32 stores.
#include <algorithm>
#include <cstdlib>

#include "../../include/omf_codec.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_dec.h"

using namespace omf;
using namespace omf::plan_layout;  // the table records and layout constants (omf_plan_layout.h)

namespace {

constexpr int kV = 16;  // float4 per thread per sub-chunk
static_assert(kSub == (int64_t)kV * kThreads * 4, "a flat item is one sub-chunk of a 256-thread workgroup");

struct DecArgs {
  const void* q;
  const float* norm;
  float* y;
  const Item* items;
  float levels;      // fl32(levels)
  float inv_levels;  // 2^-s when levels is a power of two (exact), else unused
};

// One quad's four floats from its payload (WIDTH 1: the dword raw[0]; WIDTH 4: raw[0..3]).
template <int WIDTH, bool POW2>
__device__ __forceinline__ void dec_quad(const int32_t* raw, float norm, float levels, float inv_levels,
                                         float (&yv)[4]) {
  int32_t qi[4];
  if (WIDTH == 1) {
    qsgd_split_i8(raw[0], qi);
  } else {
    qi[0] = raw[0]; qi[1] = raw[1]; qi[2] = raw[2]; qi[3] = raw[3];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) yv[c] = qsgd_dec_elem<POW2>(norm, qi[c], levels, inv_levels);
}

// Decode one sub-chunk [b, end): y = fl32(fl32(norm * q) / L) (optionally acc += y).
template <int WIDTH, bool ACC, bool POW2, bool FULL, int V = kV>
__device__ __forceinline__ void decode_sub(const DecArgs& a, int64_t b, int64_t end, float norm) {
  constexpr int R = WIDTH == 1 ? 1 : 4;  // payload dwords per quad
  int32_t raw[V][R];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int64_t e = b + 4 * ((int64_t)k * kThreads + threadIdx.x);
    if (!FULL && e + 4 > end) {
      int32_t rr[4];
      qsgd_last_quad<WIDTH>(a.q, e, end, rr);
#pragma unroll
      for (int c = 0; c < R; ++c) raw[k][c] = rr[c];
    } else if (WIDTH == 1) {  // streamed once: nontemporal
      raw[k][0] = __builtin_nontemporal_load(reinterpret_cast<const int32_t*>(reinterpret_cast<const int8_t*>(a.q) + e));
    } else {
      const i32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(reinterpret_cast<const int32_t*>(a.q) + e));
      raw[k][0] = t[0]; raw[k][1] = t[1]; raw[k][2] = t[2]; raw[k][3] = t[3];
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int64_t e = b + 4 * ((int64_t)k * kThreads + threadIdx.x);
    if (!FULL && e >= end) continue;
    float yv[4];
    dec_quad<WIDTH, POW2>(raw[k], norm, a.levels, a.inv_levels, yv);
    float* y = a.y + e;
    if (FULL || e + 4 <= end) {
      float4 o = make_float4(yv[0], yv[1], yv[2], yv[3]);
      if (ACC) {
        const f32x4_t pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(y));
        const float4 prev = make_float4(pv[0], pv[1], pv[2], pv[3]);
        o.x = __fadd_rn(prev.x, o.x); o.y = __fadd_rn(prev.y, o.y);
        o.z = __fadd_rn(prev.z, o.z); o.w = __fadd_rn(prev.w, o.w);
      }
      store_nt(y, o);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (e + c < end) y[c] = ACC ? __fadd_rn(y[c], yv[c]) : yv[c];
    }
  }
}

template <int WIDTH, bool ACC, bool POW2>
__global__ __launch_bounds__(kThreads) void qsgd_decode_flat(DecArgs a) {
  const Item it = a.items[blockIdx.x];
  const float norm = a.norm[it.tensor];
  for (int64_t b = it.begin; b < it.end; b += kSub) {
    const int64_t end = min(b + kSub, it.end);
    if (end - b == kSub) decode_sub<WIDTH, ACC, POW2, true>(a, b, end, norm);
    else decode_sub<WIDTH, ACC, POW2, false>(a, b, end, norm);
  }
}

// Decoder over arena-aligned blocks: the payload loads depend on blockIdx only, so they go out
// at once; the block's tensor (binfo, one entry per 4 Ki-element table block: tensor id, bit 31 =
// the table block lies inside it) and its norm are scalar loads in flight with them.  A block in
// a table block that crosses a tensor boundary or padding (at most nt + 1 of them) finds each
// quad's tensor and writes only its elements.  Round 5: the decode block is narrower than the
// table block — kDecQuads(W, ACC) quads per thread: 2 for an int8 payload, 1 for an int32 payload
// or an accumulate — measured on Llama-400M (interleaved): int8
// 0.298-0.304 ms against 0.331 with 4 quads, int32 0.492 against 0.550, accumulate 0.556 / 0.748
// against 0.612 / 0.807 (fewer bytes per thread, more workgroups in flight per CU).
static_assert(kDecBlk == (int64_t)4 * kThreads * 4, "4096 elements per binfo table block");
template <int WIDTH, bool ACC>
constexpr int kDecQuads = (WIDTH == 1 && !ACC) ? 2 : 1;

template <int WIDTH, bool ACC, bool POW2>
__global__ __launch_bounds__(kThreads) void qsgd_decode_arena(DecArgs a, const uint32_t* __restrict__ binfo,
                                                              const float* __restrict__ norms,
                                                              const int64_t* __restrict__ begins,
                                                              const int64_t* __restrict__ sizes, int32_t nt,
                                                              int64_t qlast, uint32_t blk0) {
  constexpr int V = kDecQuads<WIDTH, ACC>;
  const uint32_t bid = blk0 + blockIdx.x;  // a range launch starts at block blk0
  const int64_t base = (int64_t)bid * (V * kThreads * 4);
  int32_t raw[V][WIDTH == 1 ? 1 : 4];
#pragma unroll
  for (int k = 0; k < V; ++k) {  // unconditional (clamped) loads
    const int64_t e = min(base + 4 * ((int64_t)k * kThreads + threadIdx.x), qlast);
    if (WIDTH == 1) {  // default policy: 0.298 against 0.304 ms non-temporal
      raw[k][0] = *reinterpret_cast<const int32_t*>(reinterpret_cast<const int8_t*>(a.q) + e);
    } else {
      const i32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(reinterpret_cast<const int32_t*>(a.q) + e));
      raw[k][0] = t[0]; raw[k][1] = t[1]; raw[k][2] = t[2]; raw[k][3] = t[3];
    }
  }
  const uint32_t info = binfo[base / kDecBlk];
  const int32_t t0 = (int32_t)(info & 0x7fffffffu);
  if (info >> 31) {  // the whole table block lies inside tensor t0
    const float norm = norms[t0];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int64_t e = base + 4 * ((int64_t)k * kThreads + threadIdx.x);
      float yv[4];
      dec_quad<WIDTH, POW2>(raw[k], norm, a.levels, a.inv_levels, yv);
      float4 o = make_float4(yv[0], yv[1], yv[2], yv[3]);
      if (ACC) {
        const f32x4_t pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(a.y + e));
        o.x = __fadd_rn(pv[0], o.x); o.y = __fadd_rn(pv[1], o.y);
        o.z = __fadd_rn(pv[2], o.z); o.w = __fadd_rn(pv[3], o.w);
      }
      store_nt(a.y + e, o);
    }
    return;
  }
  // boundary block: each quad's tensor, element by element
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int64_t e = base + 4 * ((int64_t)k * kThreads + threadIdx.x);
    const int32_t t = qsgd_tensor_at(t0, e, begins, nt);
    const int64_t tb = begins[t], te = tb + sizes[t];
    if (e + 3 < tb || e >= te) continue;  // padding (offsets are multiples of 4: a quad never
                                          // starts before its tensor and ends inside it)
    int32_t rr[4] = {raw[k][0], WIDTH == 1 ? 0 : raw[k][1], WIDTH == 1 ? 0 : raw[k][2], WIDTH == 1 ? 0 : raw[k][3]};
    if (e + 4 > te) qsgd_last_quad<WIDTH>(a.q, e, te, rr);
    float yv[4];
    dec_quad<WIDTH, POW2>(rr, norms[t], a.levels, a.inv_levels, yv);
    for (int c = 0; c < 4; ++c)
      if (e + c < te) a.y[e + c] = ACC ? __fadd_rn(a.y[e + c], yv[c]) : yv[c];
  }
}

__global__ __launch_bounds__(kThreads) void div_f32_kernel(float* __restrict__ y, int64_t n, float d) {
  const int64_t stride = (int64_t)gridDim.x * kThreads * 4;
  for (int64_t e = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x); e < n; e += stride) {
    if (e + 4 <= n) {
      float4 v = *reinterpret_cast<float4*>(y + e);
      v.x = v.x / d; v.y = v.y / d; v.z = v.z / d; v.w = v.w / d;
      *reinterpret_cast<float4*>(y + e) = v;
    } else {
      for (int64_t i = e; i < n; ++i) y[i] = y[i] / d;
    }
  }
}

// N clients' payloads decoded and summed in one pass (omf_qsgd_decode_sum), in qsgd_decode_arena's
// shape: one workgroup per arena-aligned block of 1 Ki elements (one quad per thread; two for int8
// measured the same), all N payload quads of a thread loaded at once (unconditional, clamped), the binfo entry and the N norms scalar loads in
// flight with them, the sum in registers (client order, __fadd_rn), one non-temporal store per quad.
//   s = init ? y : +0;  s = fl32(s + dec_quad(q_c, norm_c[t]))  c = 0..N-1;  y = divisor != 0 ? s / divisor : s
// The client pointers are kernel arguments indexed at compile time (N is a template parameter: a
// runtime index into a by-value array is copied to scratch).  Boundary blocks go element by element,
// as the decoder's; with `fill` they also write the padding of [0, arena_end) (fl32(+0 / divisor), or
// +0): the bytes of memset, N accumulating decodes and omf_div_f32 over the arena.
constexpr int kSumMax = 8;  // clients per launch; omf_qsgd_decode_sum chains groups
template <int N>
struct SumArgs {
  const void* q[N];
  const float* norm[N];
  float* y;
  float levels;      // fl32(levels)
  float inv_levels;  // as DecArgs
  float divisor;     // 0: no division
  float pad_div;     // the whole call's divisor: what the padding is divided by (fill)
  int32_t init;      // the sum starts from y (else from +0: y is not read)
  int32_t fill;      // padding elements of [0, arena_end) are written
};

constexpr int64_t kSumBlk = (int64_t)kThreads * 4;  // elements per workgroup
static_assert(kDecBlk % kSumBlk == 0, "whole sum blocks per binfo table block");
template <int WIDTH, bool POW2, int N>
__global__ __launch_bounds__(kThreads) void qsgd_decode_sum_arena(SumArgs<N> a, const uint32_t* __restrict__ binfo,
                                                                  const int64_t* __restrict__ begins,
                                                                  const int64_t* __restrict__ sizes, int32_t nt,
                                                                  int64_t qlast, int64_t arena_end) {
  const int64_t base = (int64_t)blockIdx.x * kSumBlk;
  const int64_t e = base + 4 * (int64_t)threadIdx.x;
  const int64_t ec = min(e, qlast);  // unconditional (clamped) loads, every client's
  int32_t raw[N][WIDTH == 1 ? 1 : 4];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    if (WIDTH == 1) {
      raw[c][0] = *reinterpret_cast<const int32_t*>(reinterpret_cast<const int8_t*>(a.q[c]) + ec);
    } else {
      const i32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(reinterpret_cast<const int32_t*>(a.q[c]) + ec));
      raw[c][0] = t[0]; raw[c][1] = t[1]; raw[c][2] = t[2]; raw[c][3] = t[3];
    }
  }
  f32x4_t pv = {0.0f, 0.0f, 0.0f, 0.0f};
  if (a.init) pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(a.y + ec));
  const uint32_t info = binfo[base / kDecBlk];
  const int32_t t0 = (int32_t)(info & 0x7fffffffu);
  const float levels = a.levels, inv_levels = a.inv_levels;
  if (info >> 31) {  // the whole table block lies inside tensor t0
    float norm[N];
#pragma unroll
    for (int c = 0; c < N; ++c) norm[c] = a.norm[c][t0];
    float s[4] = {pv[0], pv[1], pv[2], pv[3]};
#pragma unroll
    for (int c = 0; c < N; ++c) {
      float yv[4];
      dec_quad<WIDTH, POW2>(raw[c], norm[c], levels, inv_levels, yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = __fadd_rn(s[j], yv[j]);
    }
    if (a.divisor != 0.0f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = s[j] / a.divisor;
    }
    store_nt(a.y + e, make_float4(s[0], s[1], s[2], s[3]));
    return;
  }
  // boundary block: the quad's tensor, element by element
  if (e >= arena_end) return;
  const float pad = a.pad_div != 0.0f ? 0.0f / a.pad_div : 0.0f;
  const int32_t t = qsgd_tensor_at(t0, e, begins, nt);
  const int64_t tb = begins[t], te = tb + sizes[t];
  if (e < tb || e >= te) {  // a quad of padding (offsets are multiples of 4: no tensor starts inside it)
    if (a.fill)
      for (int j = 0; j < 4; ++j)
        if (e + j < arena_end) a.y[e + j] = pad;
    return;
  }
  const bool part = e + 4 > te;  // the tensor's partial last quad
  float s[4];
  for (int j = 0; j < 4; ++j) s[j] = (a.init && e + j < te) ? a.y[e + j] : 0.0f;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    int32_t rr[4] = {raw[c][0], WIDTH == 1 ? 0 : raw[c][1], WIDTH == 1 ? 0 : raw[c][2], WIDTH == 1 ? 0 : raw[c][3]};
    if (part) {  // qsgd_last_quad's loads written out: through the helper the whole-block arm is scheduled anew
      if (WIDTH == 1) {
        const int8_t* q8 = reinterpret_cast<const int8_t*>(a.q[c]);
        uint32_t w = 0;
        for (int j = 0; j < 3; ++j)
          if (e + j < te) w |= (uint32_t)(uint8_t)q8[e + j] << (8 * j);
        rr[0] = (int32_t)w;
      } else {
        const int32_t* q32 = reinterpret_cast<const int32_t*>(a.q[c]);
        for (int j = 0; j < 3; ++j) rr[j] = e + j < te ? q32[e + j] : 0;
        rr[3] = 0;
      }
    }
    float yv[4];
    dec_quad<WIDTH, POW2>(rr, a.norm[c][t], levels, inv_levels, yv);
    for (int j = 0; j < 4; ++j) s[j] = __fadd_rn(s[j], yv[j]);
  }
  for (int j = 0; j < 4; ++j) {
    if (e + j < te) a.y[e + j] = a.divisor != 0.0f ? s[j] / a.divisor : s[j];
    else if (a.fill && e + j < arena_end) a.y[e + j] = pad;
  }
}

// The same for an arena of fewer than 4 elements (no whole quad to load): one thread per element,
// byte / dword loads, `n` clients behind a uniform guard (compile-time indices all the same).
template <int WIDTH, bool POW2>
__global__ __launch_bounds__(64) void qsgd_decode_sum_tiny(SumArgs<kSumMax> a, int32_t n,
                                                           const int64_t* __restrict__ begins,
                                                           const int64_t* __restrict__ sizes, int32_t nt,
                                                           int64_t arena_end) {
  const int64_t i = threadIdx.x;
  if (i >= arena_end) return;
  int32_t t = -1;
  for (int32_t u = 0; u < nt; ++u)
    if (i >= begins[u] && i < begins[u] + sizes[u]) t = u;
  if (t < 0) {
    if (a.fill) a.y[i] = a.pad_div != 0.0f ? 0.0f / a.pad_div : 0.0f;
    return;
  }
  float s = a.init ? a.y[i] : 0.0f;
#pragma unroll
  for (int c = 0; c < kSumMax; ++c) {
    if (c < n) {
      const int32_t q = WIDTH == 1 ? (int32_t) reinterpret_cast<const int8_t*>(a.q[c])[i]
                                   : reinterpret_cast<const int32_t*>(a.q[c])[i];
      s = __fadd_rn(s, qsgd_dec_elem<POW2>(a.norm[c][t], q, a.levels, a.inv_levels));
    }
  }
  a.y[i] = a.divisor != 0.0f ? s / a.divisor : s;
}

constexpr const char* kMisaligned = "misaligned buffer (fp32/int32 need 16 B, int8 needs 4 B alignment)";

int decode_blocks(omf_plan* p, const void* q, int32_t width, int32_t levels, const float* norm, float* y,
                  int32_t accumulate, int64_t b0, int64_t b1, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  if (width != 8 && width != 32) return fail(OMF_EINVAL, "width must be 8 or 32");
  if (levels <= 0) return fail(OMF_EINVAL, "levels must be > 0");
  if (!q || !norm || !y) return fail(OMF_EINVAL, "q, norm and y_out must be non-NULL");
  if (!aligned(y, 16) || !aligned(q, width == 8 ? 4 : 16)) return fail(OMF_EINVAL, kMisaligned);
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const LevelScale lv(levels);
  const DecArgs a{q, norm, y, p->d_flat, lv.levels, lv.inv_levels};
  b0 = std::max<int64_t>(b0, 0);
  b1 = std::min<int64_t>(b1, p->n_dec_blocks);
  if (b1 <= b0) return OMF_OK;
  const dim3 blk(kThreads);
  hipStream_t st = (hipStream_t)stream;
  // A plain decode's workgroups reserve 24 KiB of LDS each (unused): six per CU — Llama-400M 0.294-
  // 0.296 ms at s = 4 and 0.482-0.484 at s = 8 against 0.301 / 0.490 uncapped, 0.308 / 0.489 at 28 KiB
  // (DESIGN.md §3.8); OMF_DEC_LDS overrides.  Accumulating decodes keep every wave.
  static const size_t dlds = [] { const char* v = omf::knob("OMF_DEC_LDS"); return v ? (size_t)atoi(v) : (size_t)24576; }();
  // the last whole quad of the payload the caller holds (width 8: round_up(arena_end, 4) bytes
  // are not promised, so a clamped load never passes the last full quad)
  const int64_t qlast = (p->arena_end & ~(int64_t)3) - 4;  // < 0 only for arenas of < 4 elements
#define OMF_DEC(W, A, P)                                                                                         \
  do {                                                                                                           \
    if (qlast >= 0) {                                                                                            \
      const int64_t per = kDecBlk / (kDecQuads<W, A> * kThreads * 4); /* decode blocks per table block */       \
      hipLaunchKernelGGL((qsgd_decode_arena<W, A, P>), dim3((unsigned)((b1 - b0) * per)), blk, A ? 0 : dlds, st, a, \
                         (const uint32_t*)p->d_dec_binfo, norm, (const int64_t*)p->d_begins,                    \
                         (const int64_t*)p->d_sizes, p->nt, qlast, (uint32_t)(b0 * per));                       \
    } else /* a payload of < 4 elements: the item decoder's byte loads */                                          \
      hipLaunchKernelGGL((qsgd_decode_flat<W, A, P>), dim3((unsigned)p->n_flat), blk, 0, st, a);                \
  } while (0)
  if (width == 8) {
    if (accumulate) { if (lv.pow2) OMF_DEC(1, true, true); else OMF_DEC(1, true, false); }
    else { if (lv.pow2) OMF_DEC(1, false, true); else OMF_DEC(1, false, false); }
  } else {
    if (accumulate) { if (lv.pow2) OMF_DEC(4, true, true); else OMF_DEC(4, true, false); }
    else { if (lv.pow2) OMF_DEC(4, false, true); else OMF_DEC(4, false, false); }
  }
#undef OMF_DEC
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

// ---- omf_qsgd_decode_sum: one group of at most kSumMax clients per launch
struct SumCall : SumCallBase {
  const omf_plan* p;
  const void* const* q;
};

template <int N>
SumArgs<N> sum_args(const SumCall& c, int n) {
  SumArgs<N> a{};
  for (int k = 0; k < n; ++k) a.q[k] = c.q[k];
  sum_common_args(a, c, n);
  return a;
}

template <int W, bool P, int N>
void launch_sum_n(const SumCall& c) {
  const omf_plan* p = c.p;
  const int64_t qlast = (p->arena_end & ~(int64_t)3) - 4;  // the last whole quad (as decode_blocks)
  const int64_t per = kDecBlk / kSumBlk;                   // sum blocks per table block
  hipLaunchKernelGGL((qsgd_decode_sum_arena<W, P, N>), dim3((unsigned)(p->n_dec_blocks * per)), dim3(kThreads), 0,
                     c.st, sum_args<N>(c, N), (const uint32_t*)p->d_dec_binfo, (const int64_t*)p->d_begins,
                     (const int64_t*)p->d_sizes, p->nt, qlast, p->arena_end);
}

template <int W, bool P>
void launch_sum(const SumCall& c) {
  const int n = c.g.n;
  if (c.p->arena_end < 4) {  // no whole quad: the element kernel
    hipLaunchKernelGGL((qsgd_decode_sum_tiny<W, P>), dim3(1), dim3(64), 0, c.st, sum_args<kSumMax>(c, n), n,
                       (const int64_t*)c.p->d_begins, (const int64_t*)c.p->d_sizes, c.p->nt, c.p->arena_end);
    return;
  }
  with_group_size<kSumMax>(n, [&](auto N) { launch_sum_n<W, P, N()>(c); });
}

}  // namespace

extern "C" {

int omf_qsgd_decode(omf_plan* p, const void* q, int32_t width, int32_t levels, const float* norm, float* y,
                    int32_t accumulate, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  return decode_blocks(p, q, width, levels, norm, y, accumulate, 0, p->n_dec_blocks, stream);
}

int omf_qsgd_decode_range(omf_plan* p, const void* q, int32_t width, int32_t levels, const float* norm, float* y,
                          int32_t accumulate, int64_t elem_begin, int64_t elem_end, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  if (elem_begin < 0 || elem_end < elem_begin) return fail(OMF_EINVAL, "omf_qsgd_decode_range: bad element range");
  if (elem_end == elem_begin) return OMF_OK;  // an empty range overlaps no block, wherever it lies
  if (p->arena_end < 4)  // the item decoder of tiny payloads has no block ranges: its one block, whole
    return decode_blocks(p, q, width, levels, norm, y, accumulate, 0, elem_begin < kDecBlk ? p->n_dec_blocks : 0, stream);
  return decode_blocks(p, q, width, levels, norm, y, accumulate, elem_begin / kDecBlk,
                       (elem_end + kDecBlk - 1) / kDecBlk, stream);
}

int omf_div_f32(float* y, int64_t n, float divisor, void* stream) {
  if (n < 0 || (n > 0 && !y)) return fail(OMF_EINVAL, "omf_div_f32: bad arguments");
  if (n == 0) return OMF_OK;
  if (!aligned(y, 16)) return fail(OMF_EINVAL, "omf_div_f32: y must be 16-byte aligned");
  const int64_t blocks = std::min<int64_t>((n + 4 * kThreads - 1) / (4 * kThreads), 8192);
  hipLaunchKernelGGL(div_f32_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, y, n, divisor);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf_qsgd_decode_sum(omf_plan* p, const void* const* q, const float* const* norm, int32_t nclients, int32_t width,
                        int32_t levels, float* y, int32_t init, float divisor, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  if (width != 8 && width != 32) return fail(OMF_EINVAL, "width must be 8 or 32");
  if (levels <= 0) return fail(OMF_EINVAL, "levels must be > 0");
  if (nclients < 1) return fail(OMF_EINVAL, "omf_qsgd_decode_sum: nclients must be >= 1");
  if (!q || !norm || !y) return fail(OMF_EINVAL, "q, norm and y_out must be non-NULL");
  if (!aligned(y, 16)) return fail(OMF_EINVAL, kMisaligned);
  const size_t ybytes = (size_t)p->arena_end * 4;
  const size_t qbytes = width == 8 ? (size_t)((p->arena_end + 3) & ~(int64_t)3) : (size_t)p->arena_end * 4;
  for (int32_t k = 0; k < nclients; ++k) {
    if (!q[k] || !norm[k]) return fail(OMF_EINVAL, "omf_qsgd_decode_sum: a NULL entry in q or norm");
    if (!aligned(q[k], width == 8 ? 4 : 16)) return fail(OMF_EINVAL, kMisaligned);
    if (overlaps(y, ybytes, q[k], qbytes) || overlaps(y, ybytes, norm[k], (size_t)p->nt * 4))
      return fail(OMF_EINVAL, "omf_qsgd_decode_sum: y_out overlaps a payload or norm buffer");
  }
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const LevelScale lv(levels);
  SumCall c;
  c.p = p; c.y = y; c.st = (hipStream_t)stream; c.levels = lv.levels; c.inv_levels = lv.inv_levels;
  for (int32_t k0 = 0; k0 < nclients; k0 += kSumMax) {  // the chained groups (sum_group, omf_qsgd_dec.h)
    c.g = sum_group(nclients, kSumMax, init, divisor, k0);
    c.q = q + k0; c.norm = norm + k0;
    if (width == 8) {
      if (lv.pow2) launch_sum<1, true>(c); else launch_sum<1, false>(c);
    } else {
      if (lv.pow2) launch_sum<4, true>(c); else launch_sum<4, false>(c);
    }
    OMF_HIP(hipGetLastError());
  }
  return OMF_OK;
}

}  // extern "C"
