// omf_topk_qval.hip — the opt-in quantised Top-K value wire ("TopKQuantPackedCompression"), MI355X (gfx950).
//
// NOT reference-compatible: a new compression_type a sender uses only when asked to.  The k selected fp32
// values of a tensor become QSGD levels against the tensor's scale m = max |v| (exact, and independent of the
// reduction order; an L2 norm would put k values of similar size at 1 / sqrt k, where a level is almost
// always 0): q by the encoder's rule (Divisor(m), qsgd_quad: omf_qsgd_dev.h) with L = 2^s levels and the
// encoder's Philox stream, "element" read as the position in the tensor's selection (oracle/philox.py), the
// code q + L in b = s + 2 bits, packed as the indices are (pack_group / unpack_group, omf_topk_layout.h): a
// group of 32 consecutive values of one tensor is b whole words, group g of the selection at word g b.  The
// receiver restores d = fl32(fl32(m q) / L) (qsgd_dec_elem: omf_qsgd_dec.h); the sender's error feedback
// takes e = fl32(v - d) at the value's own slot of the residual arena, which the encode left zero.
//
// Three kernels of one thread per group, 256 per workgroup, as omf_topk_pack.hip's: the scales (an unsigned
// maximum of the bits of |v|: NaN bits sort above infinity's, so an unusable scale shows), the quantiser and
// the dequantiser.  A scale is unusable when it is NaN, infinite or above FLT_MAX / L (m L would overflow):
// the quantiser writes nothing for that tensor and the sender keeps its fp32 values on the packed-index
// wire; a negative scale marks such a tensor for the dequantiser, which then leaves its values alone.
#include <cfloat>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/omf_codec.h"
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_dec.h"  // aligned, overlaps, qsgd_dec_elem
#include "omf_qsgd_dev.h"  // Divisor, qsgd_quad
#include "omf_topk_dev.h"
#include "omf_topk_layout.h"

using namespace omf;
using namespace omf::topk_layout;

namespace {

// What a thread knows of its group: the tensor, the group's live values (1..32), its first value's place in
// the selection arena and in the tensor's selection.
struct GroupAt {
  int t, nv;
  int64_t o0, p0;
};
__device__ __forceinline__ GroupAt group_at(const int64_t* __restrict__ koff, const uint32_t* __restrict__ goff,
                                            uint32_t* s_goff, int nt, int64_t g) {
  GroupAt a;
  a.t = group_tensor(goff, s_goff, nt, g);
  a.p0 = kPackGroup * (g - (int64_t)goff[a.t]);
  const int64_t k0 = koff[a.t];
  a.nv = (int)min((int64_t)kPackGroup, koff[a.t + 1] - k0 - a.p0);
  a.o0 = k0 + a.p0;
  return a;
}

// scales[t] = max |v| over tensor t's selection, as bits: a vector atomic unsigned maximum into a word the
// call cleared, whatever the launch shape (the maximum is exact and order-free).  A thread whose maximum
// does not exceed what the word already holds has nothing to add.
__global__ __launch_bounds__(kThreads) void topk_qval_scales(const float* __restrict__ values,
                                                             const int64_t* __restrict__ koff,
                                                             const uint32_t* __restrict__ goff, int nt,
                                                             int64_t groups, uint32_t* __restrict__ scales) {
  __shared__ uint32_t s_goff[kArenaMaxTensors + 1];
  stage_goff(goff, s_goff, nt);
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= groups) return;
  const GroupAt a = group_at(koff, goff, s_goff, nt, g);
  const float* src = values + a.o0;
  uint32_t mx = 0;
#pragma unroll
  for (int i = 0; i < kPackGroup; ++i)
    if (i < a.nv) mx = max(mx, __float_as_uint(src[i]) & 0x7FFFFFFFu);
  if (mx > __hip_atomic_load(&scales[a.t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    __hip_atomic_fetch_max(&scales[a.t], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The four draws of quad `quad` (elements 4 quad .. 4 quad + 3 of the tensor's selection): Philox group
// G = ((row >> 2) << 8) | (quad & 255) with row = quad >> 8, and of its 12 words the three from word
// 3 (row & 3) on — one Philox call, or two where the three words straddle calls (oracle/philox.py).
struct DrawKey {
  uint32_t seed_lo, seed_hi, offset;
};
__device__ __forceinline__ float4 quad_draws(const DrawKey& k, int64_t quad, int t) {
  const uint64_t row = (uint64_t)quad >> 8;
  const uint64_t G = ((row >> 2) << 8) | ((uint64_t)quad & 255u);
  const uint32_t first = 3u * (uint32_t)(row & 3);  // first word of the 12
  const uint32_t ca = first >> 2, cb = (first + 2) >> 2, s = first & 3;
  auto call = [&](uint32_t c) {
    const uint64_t ctr = 3 * G + c;
    return philox4x32_10(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)t, k.offset), k.seed_lo, k.seed_hi);
  };
  const uint4 A = call(ca);
  uint4 B = A;
  if (cb != ca) B = call(cb);
  // words s, s + 1, s + 2 of {A.x, A.y, A.z, A.w, B.x, B.y}
  const uint32_t w0 = s == 0 ? A.x : s == 1 ? A.y : s == 2 ? A.z : A.w;
  const uint32_t w1 = s == 0 ? A.y : s == 1 ? A.z : s == 2 ? A.w : B.x;
  const uint32_t w2 = s == 0 ? A.z : s == 1 ? A.w : s == 2 ? B.x : B.y;
  return u24x4(w0, w1, w2);
}

// One thread per group: its values (and, with a residual, its indices) loaded before any store, quantised
// quad by quad with the encoder's rule, packed into b whole words at word g b — the codes after the tensor's
// k_t-th value are 0 — and the quantisation error stored at each value's own residual slot (an index
// outside [0, n_t) stores nothing).  Scale 0: every code is L, no draw, no residual store.  An unusable
// scale (not in [0, lmax]): nothing at all.
__global__ __launch_bounds__(kThreads) void topk_qval_quant(
    const float* __restrict__ values, const int64_t* __restrict__ indices, const int64_t* __restrict__ koff,
    const uint32_t* __restrict__ goff, const int64_t* __restrict__ sizes, const int64_t* __restrict__ begins,
    const float* __restrict__ scales, int nt, int64_t groups, int b, float L, float inv_L, float lmax, DrawKey key,
    float* __restrict__ residual, uint32_t* __restrict__ packed) {
  __shared__ uint32_t s_goff[kArenaMaxTensors + 1];
  stage_goff(goff, s_goff, nt);
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= groups) return;
  const GroupAt a = group_at(koff, goff, s_goff, nt, g);
  const float m = scales[a.t];
  if (!(m >= 0.0f && m <= lmax)) return;
  const float* src = values + a.o0;
  float v[kPackGroup];
#pragma unroll
  for (int i = 0; i < kPackGroup; ++i) v[i] = i < a.nv ? src[i] : 0.0f;
  const bool ef = residual != nullptr && m != 0.0f;
  int64_t ix[kPackGroup];
  if (ef) {
    const int64_t* isrc = indices + a.o0;
#pragma unroll
    for (int i = 0; i < kPackGroup; ++i) ix[i] = i < a.nv ? isrc[i] : -1;
  }
  const int32_t Li = (int32_t)L;
  uint32_t code[kPackGroup];
  if (m == 0.0f) {
#pragma unroll
    for (int i = 0; i < kPackGroup; ++i) code[i] = (uint32_t)Li;
  } else {
    const Divisor dv(m);
    const int64_t n = sizes[a.t];
    float* res = ef ? residual + begins[a.t] : nullptr;
#pragma unroll
    for (int q4 = 0; q4 < kPackGroup / 4; ++q4) {
      const float4 u = quad_draws(key, (a.p0 >> 2) + q4, a.t);
      int32_t lv[4];
      // |v| <= m, so |v / m| L <= L: no level can reach the int64 overflow the big check is for
      qsgd_quad<false>(make_float4(v[4 * q4], v[4 * q4 + 1], v[4 * q4 + 2], v[4 * q4 + 3]), u, dv, L, false, lv);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = 4 * q4 + c;
        code[i] = (uint32_t)(lv[c] + Li);
        if (ef && i < a.nv && ix[i] >= 0 && ix[i] < n)
          res[ix[i]] = __fsub_rn(v[i], qsgd_dec_elem<true>(m, lv[c], L, inv_L));
      }
    }
  }
  pack_group(code, a.nv, b, packed + value_group_word(g, b));
}

// One thread per group restores the group's first nv values (reading only the words that hold their codes)
// into its 33-word row of an LDS tile; then each half wave stores one group's values, 32 consecutive floats,
// so the stores are lane-contiguous.  A tensor with a negative scale is skipped: its fp32 values are in
// place already.  Nothing past a tensor's k_t-th value is written.
constexpr int kRow = kPackGroup + 1;
__global__ __launch_bounds__(kThreads) void topk_qval_dequant(const uint32_t* __restrict__ packed,
                                                              const int64_t* __restrict__ koff,
                                                              const uint32_t* __restrict__ goff,
                                                              const float* __restrict__ scales, int nt,
                                                              int64_t groups, int b, float L, float inv_L,
                                                              float* __restrict__ values) {
  __shared__ uint32_t s_goff[kArenaMaxTensors + 1];
  __shared__ float tile[kRow * kThreads];
  __shared__ int64_t s_o0[kThreads];
  __shared__ int32_t s_nv[kThreads];
  stage_goff(goff, s_goff, nt);
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int nv = 0;
  int64_t o0 = 0;
  if (g < groups) {
    const GroupAt a = group_at(koff, goff, s_goff, nt, g);
    const float m = scales[a.t];
    o0 = a.o0;
    if (!(m < 0.0f)) {
      nv = a.nv;
      uint32_t c[kPackGroup] = {};
      unpack_group(packed + value_group_word(g, b), nv, b, c);
      const int32_t Li = (int32_t)L;
#pragma unroll
      for (int i = 0; i < kPackGroup; ++i)
        if (i < nv) tile[kRow * threadIdx.x + i] = qsgd_dec_elem<true>(m, (int32_t)c[i] - Li, L, inv_L);
    }
  }
  s_o0[threadIdx.x] = o0;
  s_nv[threadIdx.x] = nv;
  __syncthreads();
  const int lane = threadIdx.x & (kPackGroup - 1);
  for (int gl = threadIdx.x / kPackGroup; gl < kThreads; gl += kThreads / kPackGroup)
    if (lane < s_nv[gl]) values[s_o0[gl] + lane] = tile[kRow * gl + lane];
}

// What the three calls share: the counts' tables, the code width and the level count.
struct QvalArgs {
  PackArgs p;
  int32_t b = 0;
  float L = 0.0f;
  dim3 grid;
};
int qval_args(omf_plan* plan, const int64_t* counts, int32_t bit_width, QvalArgs* out) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  out->b = value_code_bits(bit_width);
  if (out->b < 0) return fail(OMF_EINVAL, "bit_width must be in 1..8");
  out->L = (float)(1 << bit_width);
  if (int r = topk_pack_args(plan, counts, &out->p)) return r;
  out->grid = dim3((unsigned)((out->p.groups + kThreads - 1) / kThreads));
  return OMF_OK;
}

}  // namespace

extern "C" {

int64_t omf_topk_value_words(omf_plan* plan, const int64_t* counts, int32_t bit_width) {
  int64_t ktot = 0;
  const int32_t b = value_code_bits(bit_width);
  if (!plan || b < 0 || topk_check_counts(plan, counts, &ktot)) return -1;
  const PackTables h = pack_tables_host(plan->sizes, counts);
  return h.words < 0 ? -1 : value_words(h, b);
}

int omf_topk_value_scales(omf_plan* plan, const int64_t* counts, const float* values, float* scales, void* stream) {
  QvalArgs a;
  if (int r = qval_args(plan, counts, kQvalMinBits, &a)) return r;
  if (!scales) return fail(OMF_EINVAL, "values and scales must be non-NULL");
  if (!aligned(scales, 4)) return fail(OMF_EINVAL, "values and scales must be 4-byte aligned");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  OMF_HIP(hipMemsetAsync(scales, 0, 4 * (size_t)plan->nt, (hipStream_t)stream));  // a tensor without a value: 0
  if (a.p.ktot == 0) return OMF_OK;
  if (!values) return fail(OMF_EINVAL, "values and scales must be non-NULL");
  if (!aligned(values, 4)) return fail(OMF_EINVAL, "values and scales must be 4-byte aligned");
  if (overlaps(values, 4 * (size_t)a.p.ktot, scales, 4 * (size_t)plan->nt))
    return fail(OMF_EINVAL, "values and scales overlap");
  hipLaunchKernelGGL(topk_qval_scales, a.grid, dim3(kThreads), 0, (hipStream_t)stream, values,
                     (const int64_t*)a.p.dev.koff, (const uint32_t*)a.p.dev.goff, (int)plan->nt, a.p.groups,
                     reinterpret_cast<uint32_t*>(scales));
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf_topk_quantize_values(omf_plan* plan, const int64_t* counts, const float* values, const int64_t* indices,
                             const float* scales, int32_t bit_width, uint64_t seed, uint64_t offset, float* residual,
                             uint32_t* packed_values, void* stream) {
  QvalArgs a;
  if (int r = qval_args(plan, counts, bit_width, &a)) return r;
  if (a.p.ktot == 0) return OMF_OK;
  if (!values || !scales || !packed_values || (residual && !indices))
    return fail(OMF_EINVAL, "values, scales and packed_values (and indices, with a residual) must be non-NULL");
  if (!aligned(values, 4) || !aligned(scales, 4) || !aligned(packed_values, 4) || !aligned(residual, 4) ||
      !aligned(indices, 8))
    return fail(OMF_EINVAL, "values, scales, residual and packed_values must be 4-byte, indices 8-byte aligned");
  const size_t vb = 4 * (size_t)a.p.ktot, ib = indices ? 8 * (size_t)a.p.ktot : 0, sb = 4 * (size_t)plan->nt;
  const size_t pb = 4 * (size_t)value_group_word(a.p.groups, a.b), rb = residual ? 4 * (size_t)plan->arena_end : 0;
  if (overlaps(packed_values, pb, values, vb) || overlaps(packed_values, pb, indices, ib) ||
      overlaps(packed_values, pb, scales, sb) || overlaps(packed_values, pb, residual, rb))
    return fail(OMF_EINVAL, "packed_values overlaps an input or the residual");
  if (overlaps(residual, rb, values, vb) || overlaps(residual, rb, indices, ib) || overlaps(residual, rb, scales, sb))
    return fail(OMF_EINVAL, "residual overlaps an input");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const DrawKey key{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset};
  hipLaunchKernelGGL(topk_qval_quant, a.grid, dim3(kThreads), 0, (hipStream_t)stream, values, indices,
                     (const int64_t*)a.p.dev.koff, (const uint32_t*)a.p.dev.goff, (const int64_t*)plan->d_sizes,
                     (const int64_t*)plan->d_begins, scales, (int)plan->nt, a.p.groups, (int)a.b, a.L, 1.0f / a.L,
                     FLT_MAX / a.L, key, residual, packed_values);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

int omf_topk_dequantize_values(omf_plan* plan, const int64_t* counts, const uint32_t* packed_values,
                               const float* scales, int32_t bit_width, float* values, void* stream) {
  QvalArgs a;
  if (int r = qval_args(plan, counts, bit_width, &a)) return r;
  if (a.p.ktot == 0) return OMF_OK;
  if (!packed_values || !scales || !values) return fail(OMF_EINVAL, "packed_values, scales and values must be non-NULL");
  if (!aligned(packed_values, 4) || !aligned(scales, 4) || !aligned(values, 4))
    return fail(OMF_EINVAL, "packed_values, scales and values must be 4-byte aligned");
  const size_t vb = 4 * (size_t)a.p.ktot, pb = 4 * (size_t)value_group_word(a.p.groups, a.b);
  if (overlaps(values, vb, packed_values, pb) || overlaps(values, vb, scales, 4 * (size_t)plan->nt))
    return fail(OMF_EINVAL, "values overlaps packed_values or scales");
  DeviceGuard g(plan->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  hipLaunchKernelGGL(topk_qval_dequant, a.grid, dim3(kThreads), 0, (hipStream_t)stream, packed_values,
                     (const int64_t*)a.p.dev.koff, (const uint32_t*)a.p.dev.goff, scales, (int)plan->nt, a.p.groups,
                     (int)a.b, a.L, 1.0f / a.L, values);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

}  // extern "C"
