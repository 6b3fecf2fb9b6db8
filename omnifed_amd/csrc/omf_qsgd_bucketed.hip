// omf_qsgd_bucketed.hip — QSGD with bucket norms, MI355X (gfx950): the single-read bucketed encoder, the
// bucketed decoder and the K-client decode-and-sum, with their host side.  The definition (bucket size d, the
// bucket-norm arena's layout, the summation order of a bucket's norm) is omf_qsgd_bucket.h; the element math,
// the row loads, the draws and the payload stores are the other encoders' (omf_qsgd_enc.h, omf_qsgd_dev.h),
// the decode rules and the sums' chaining the other decoders' (omf_qsgd_dec.h).  DESIGN.md §3.4c.
//
// Kernel map:
//   qsgd_bucket_encode<WIDTH, HAS_U, V>   one 256-thread workgroup per block of V rows (V * 1024 elements) of a
//                    flat 16 Ki item.  Row k of the block at b is the quad at b + 4 (k 256 + tid), as in every
//                    encoder, and blocks start a multiple of 4096 elements after their tensor's begin, so a
//                    bucket is d / 4 consecutive lanes of one row (d <= 1024) or 2 / 4 whole rows of one
//                    block: x is loaded once (16 B per lane and row, non-temporal) and stays in registers,
//                    each lane squares and sums its quad, bucket_sums (omf_qsgd_bucket.h) leaves the bucket's
//                    sum in every lane of the bucket — DPP / permlane inside a wave, one LDS exchange across
//                    waves from d = 512 up, an in-thread add across rows above 1024 — the bucket's first lane
//                    stores the norm, and every lane quantises its quads against its own bucket's norm.
//                    No workgroup waits for another: no polling, no ticket, no atomic, no timeout.
//                    The default instances (V = 4) take d at compile time (LOGD = 6 .. 12: the butterfly's
//                    branches fold away; measured no slower at any size and faster from d = 1024 up, DESIGN.md
//                    §3.4c); LOGD = 0 takes it as a kernel argument (wave-uniform branches): the V = 8 / 16 and
//                    one V = 4 instance, the measurement's other sides (omf_plan_set_bucket_rows).
//                    A NULL q stops after the norms (omf_qsgd_norms_bucketed).
//   qsgd_bucket_decode_sum<WIDTH, POW2, N>  N clients' payloads decoded and summed in qsgd_decode_sum_arena's
//                    shape (omf_qsgd_recv.hip): one quad per thread over arena-aligned blocks of 1 Ki elements,
//                    every quad's norm loaded from bnorm[boff[t] + ((e - tbegin) >> log2 d)] (a quad never
//                    straddles buckets: offsets and d are multiples of 4).  The plain decode is its N = 1
//                    launch that starts from y (accumulate) or from +0, without the padding fill.
//   qsgd_bucket_sum_tiny   the same for an arena of fewer than 4 elements (no whole quad to load).
//
// HBM-bound; no MFMA (no contraction).  Encode traffic: 4 B read, 1 B (int8) + 4 / d B written per element.
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/omf_codec.h"
#include "../../include/omf_codec_experimental.h"
#include "omf_bracket.h"  // EncCall, enc_args, launch_kernel
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_bucket.h"
#include "omf_qsgd_dec.h"
#include "omf_qsgd_enc.h"

using namespace omf;
using namespace omf::plan_layout;

namespace {

// ---------------------------------------------------------------- encoder

// One block [b, end) of V rows of tensor `tensor` (begins at tbegin; its norms at nbase of the bucket arena):
// bucket_front and quant_rows (omf_qsgd_bucket.h) with the int8 / int32 wire's store (store_quad).
template <int WIDTH, bool HAS_U, bool FULL, int V>
__device__ __forceinline__ void bucket_block(const EncArgs& a, int64_t b, int64_t end, int64_t tbegin, int32_t tensor,
                                             int64_t nbase, int logd, float (*xch)[kWaves]) {
  float4 v[V];
  float norm[V];
  bucket_front<FULL, V>(a, b, end, tbegin, nbase, logd, xch, v, norm);
  if (!a.q) return;  // norms only (uniform)
  quant_rows<HAS_U, FULL, V>(v, a, b, end, tbegin, tensor, norm,
                             [&](int, int64_t e, const int32_t (&qq)[4]) { store_quad<WIDTH, FULL>(a, e, end, qq); });
}

// LOGD: log2 d at compile time (the butterfly's branches fold away), or 0: the kernel argument.
template <int WIDTH, bool HAS_U, int V, int LOGD>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_encode(EncArgs a, const int64_t* __restrict__ boff, int logd_arg) {
  const int logd = LOGD ? LOGD : logd_arg;
  constexpr int PER = (int)(kSub / ((int64_t)V * 1024));  // blocks per flat item
  __shared__ float xch[V][kWaves];
  const Item it = a.items[blockIdx.x / PER];
  const int64_t b = it.begin + (int64_t)(blockIdx.x % PER) * V * 1024;
  if (b >= it.end) return;
  const int64_t end = min(b + (int64_t)V * 1024, it.end);
  const int64_t tbegin = a.tinfo[it.tensor].begin;
  const int64_t nbase = boff[it.tensor];
  if (end - b == (int64_t)V * 1024) bucket_block<WIDTH, HAS_U, true, V>(a, b, end, tbegin, it.tensor, nbase, logd, xch);
  else bucket_block<WIDTH, HAS_U, false, V>(a, b, end, tbegin, it.tensor, nbase, logd, xch);
}

using BucketKernel = void (*)(EncArgs, const int64_t*, int);

template <int V, int LOGD = 0>
BucketKernel encode_kernel(bool int32_wire, bool has_u) {
  static const BucketKernel kern[2][2] = {{qsgd_bucket_encode<1, false, V, LOGD>, qsgd_bucket_encode<1, true, V, LOGD>},
                                          {qsgd_bucket_encode<4, false, V, LOGD>, qsgd_bucket_encode<4, true, V, LOGD>}};
  return kern[int32_wire][has_u];
}

// The 4-row kernel with d at compile time.
BucketKernel encode_kernel_static(int logd, bool w, bool u) {
  switch (logd) {
    case 6: return encode_kernel<4, 6>(w, u);
    case 7: return encode_kernel<4, 7>(w, u);
    case 8: return encode_kernel<4, 8>(w, u);
    case 9: return encode_kernel<4, 9>(w, u);
    case 10: return encode_kernel<4, 10>(w, u);
    case 11: return encode_kernel<4, 11>(w, u);
    default: return encode_kernel<4, 12>(w, u);
  }
}

// ---------------------------------------------------------------- decode and sum

constexpr int64_t kSumBlk = (int64_t)kThreads * 4;  // elements per workgroup
static_assert(kDecBlk % kSumBlk == 0, "whole sum blocks per binfo table block");

//   s = init ? y : +0;  s = fl32(s + dec_quad(q_c, bnorm_c[bucket]))  c = 0..N-1;  y = divisor != 0 ? s / divisor : s
// All N payload quads of a thread are loaded at once (unconditional, clamped to the payload's last whole
// quad); the binfo entry, the tensor's begin and boff are scalar loads in flight with them, the N norms one
// gather each (d / 4 lanes share an address).  Boundary blocks go element by element; with `fill` they also
// write the padding of [0, arena_end).
template <int WIDTH, bool POW2, int N>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_decode_sum(BSumArgs<N> a, const uint32_t* __restrict__ binfo,
                                                                   const int64_t* __restrict__ begins,
                                                                   const int64_t* __restrict__ sizes,
                                                                   const int64_t* __restrict__ boff, int logd,
                                                                   int32_t nt, int64_t qlast, int64_t arena_end) {
  const int64_t base = (int64_t)blockIdx.x * kSumBlk;
  const int64_t e = base + 4 * (int64_t)threadIdx.x;
  const int64_t ec = min(e, qlast);
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
    const int64_t ni = boff[t0] + ((e - begins[t0]) >> logd);
    float norm[N];
#pragma unroll
    for (int c = 0; c < N; ++c) norm[c] = a.norm[c][ni];
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
  const int64_t ni = boff[t] + ((e - tb) >> logd);
  const bool part = e + 4 > te;  // the tensor's partial last quad
  float s[4];
  for (int j = 0; j < 4; ++j) s[j] = (a.init && e + j < te) ? a.y[e + j] : 0.0f;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    int32_t rr[4] = {raw[c][0], WIDTH == 1 ? 0 : raw[c][1], WIDTH == 1 ? 0 : raw[c][2], WIDTH == 1 ? 0 : raw[c][3]};
    if (part) qsgd_last_quad<WIDTH>(a.q[c], e, te, rr);
    float yv[4];
    dec_quad<WIDTH, POW2>(rr, a.norm[c][ni], levels, inv_levels, yv);
    for (int j = 0; j < 4; ++j) s[j] = __fadd_rn(s[j], yv[j]);
  }
  for (int j = 0; j < 4; ++j) {
    if (e + j < te) a.y[e + j] = a.divisor != 0.0f ? s[j] / a.divisor : s[j];
    else if (a.fill && e + j < arena_end) a.y[e + j] = pad;
  }
}

// An arena of fewer than 4 elements (one tensor at offset 0, one bucket): one thread per element, byte /
// dword loads, `n` clients behind a uniform guard.
template <int WIDTH, bool POW2>
__global__ __launch_bounds__(64) void qsgd_bucket_sum_tiny(BSumArgs<kBucketSumMax> a, int32_t n,
                                                           const int64_t* __restrict__ begins,
                                                           const int64_t* __restrict__ sizes,
                                                           const int64_t* __restrict__ boff, int32_t nt,
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
  const int64_t ni = boff[t];  // i - begins[t] < 4 <= d: the tensor's first bucket
  float s = a.init ? a.y[i] : 0.0f;
#pragma unroll
  for (int c = 0; c < kBucketSumMax; ++c) {
    if (c < n) {
      const int32_t q = WIDTH == 1 ? (int32_t) reinterpret_cast<const int8_t*>(a.q[c])[i]
                                   : reinterpret_cast<const int32_t*>(a.q[c])[i];
      s = __fadd_rn(s, qsgd_dec_elem<POW2>(a.norm[c][ni], q, a.levels, a.inv_levels));
    }
  }
  a.y[i] = a.divisor != 0.0f ? s / a.divisor : s;
}

// ---------------------------------------------------------------- host side

int encode_bucketed(omf_plan* p, const float* x, float alpha, int32_t s, int64_t d, const float* u, uint64_t seed,
                    uint64_t offset, const float* bnorm_in, void* q, float* bnorm_out, bool norm_only, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd = bucket::log2_size(d);
  if (logd < 0) return fail(OMF_EINVAL, kBucketBadSize);
  if (s < 0 || s > 30) return fail(OMF_EINVAL, "bit_width must be in [0, 30] (levels = 2^bit_width is an int32 on the wire)");
  const int width = (1 << s) <= 127 ? 1 : 4;
  if (!x || !bnorm_out || (!norm_only && !q)) return fail(OMF_EINVAL, "x, q and bnorm_out must be non-NULL");
  if (!aligned(x, 16) || (u && !aligned(u, 16)) || (q && !aligned(q, width == 1 ? 4 : 16)))
    return fail(OMF_EINVAL, kBucketMisaligned);
  if (!aligned(bnorm_out, 4) || (bnorm_in && !aligned(bnorm_in, 4))) return fail(OMF_EINVAL, "misaligned bucket norms");
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const int64_t* boff = nullptr;
  int64_t nb = 0;
  if (int r = bucket_tables(p, logd, &boff, &nb)) return r;
  const hipStream_t st = (hipStream_t)stream;
  EncArgs a = enc_args(p, EncCall{x, alpha, s, u, seed, offset, bnorm_in, norm_only ? nullptr : q, bnorm_out, norm_only,
                                  st, 0.0f, nullptr, 0u, nullptr, width});
  a.items = p->d_flat;
  a.tinfo = p->d_tinfo[0];
  const int rows = p->bucket_rows;
  const unsigned blocks = (unsigned)(p->n_flat * (kSub / (rows * 1024)));
  const bool w = width == 4, hu = u != nullptr;
  const BucketKernel k = rows == 4 ? (p->bucket_static_d ? encode_kernel_static(logd, w, hu) : encode_kernel<4>(w, hu))
                                   : (rows == 16 ? encode_kernel<16>(w, hu) : encode_kernel<8>(w, hu));
  launch_kernel(k, dim3(blocks), dim3(kThreads), 0, st, a, boff, logd);
  OMF_HIP(hipGetLastError());
  if (!norm_only) p->last_encoder = kEncBucketed;
  return OMF_OK;
}

struct BSumCall : SumCallBase {
  const omf_plan* p;
  const void* const* q;
  const int64_t* boff;
  int logd;
};

template <int N>
BSumArgs<N> sum_args(const BSumCall& c, int n) {
  BSumArgs<N> a{};
  for (int k = 0; k < n; ++k) a.q[k] = c.q[k];
  sum_common_args(a, c, n);
  return a;
}

template <int W, bool P>
void launch_sum(const BSumCall& c) {
  const omf_plan* p = c.p;
  const int n = c.g.n;
  if (p->arena_end < 4) {  // no whole quad: the element kernel
    hipLaunchKernelGGL((qsgd_bucket_sum_tiny<W, P>), dim3(1), dim3(64), 0, c.st, sum_args<kBucketSumMax>(c, n), n,
                       (const int64_t*)p->d_begins, (const int64_t*)p->d_sizes, c.boff, p->nt, p->arena_end);
    return;
  }
  const int64_t qlast = (p->arena_end & ~(int64_t)3) - 4;  // the last whole quad of a payload
  const unsigned blocks = (unsigned)(p->n_dec_blocks * (kDecBlk / kSumBlk));
  with_group_size<kBucketSumMax>(n, [&](auto N) {
    hipLaunchKernelGGL((qsgd_bucket_decode_sum<W, P, N()>), dim3(blocks), dim3(kThreads), 0, c.st, sum_args<N()>(c, N()),
                       (const uint32_t*)p->d_dec_binfo, (const int64_t*)p->d_begins, (const int64_t*)p->d_sizes, c.boff,
                       c.logd, p->nt, qlast, p->arena_end);
  });
}

// The checks both receive calls share, then the chained groups.  `plain`: omf_qsgd_decode_bucketed's one
// client, which never fills the padding.
int sum_bucketed(omf_plan* p, const void* const* q, const float* const* bnorm, int32_t nclients, int32_t width,
                 int32_t levels, int64_t d, float* y, int32_t init, float divisor, bool plain, void* stream) {
  const std::string who = plain ? "omf_qsgd_decode_bucketed" : "omf_qsgd_decode_sum_bucketed";
  int logd = 0;
  if (int r = bucket_sum_checks(p, q, bnorm, nclients, width, levels, d, y, plain, who, &logd)) return r;
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const LevelScale lv(levels);
  BSumCall c;
  int64_t nb_table = 0;
  if (int r = bucket_tables(p, logd, &c.boff, &nb_table)) return r;
  c.p = p; c.y = y; c.st = (hipStream_t)stream; c.levels = lv.levels; c.inv_levels = lv.inv_levels; c.logd = logd;
  for (int32_t k0 = 0; k0 < nclients; k0 += kBucketSumMax) {
    c.g = sum_group(nclients, kBucketSumMax, init, divisor, k0);
    if (plain) c.g.fill = 0;
    c.q = q + k0; c.norm = bnorm + k0;
    if (width == 8) {
      if (lv.pow2) launch_sum<1, true>(c); else launch_sum<1, false>(c);
    } else {
      if (lv.pow2) launch_sum<4, true>(c); else launch_sum<4, false>(c);
    }
    OMF_HIP(hipGetLastError());
  }
  return OMF_OK;
}

}  // namespace

extern "C" {

int64_t omf_qsgd_bucket_count(const omf_plan* plan, int64_t bucket_size) {
  const int logd = bucket::log2_size(bucket_size);
  if (!plan || logd < 0) return -1;
  return bucket::offsets(plan->sizes.data(), plan->nt, logd, nullptr);
}

int omf_qsgd_encode_bucketed(omf_plan* plan, const float* x, float alpha, int32_t bit_width, int64_t bucket_size,
                             const float* u, uint64_t seed, uint64_t offset, const float* bnorm_in, void* q_out,
                             float* bnorm_out, void* stream) {
  return encode_bucketed(plan, x, alpha, bit_width, bucket_size, u, seed, offset, bnorm_in, q_out, bnorm_out, false, stream);
}

int omf_qsgd_norms_bucketed(omf_plan* plan, const float* x, float alpha, int64_t bucket_size, float* bnorm_out,
                            void* stream) {
  return encode_bucketed(plan, x, alpha, 0, bucket_size, nullptr, 0, 0, nullptr, nullptr, bnorm_out, true, stream);
}

int omf_qsgd_decode_bucketed(omf_plan* plan, const void* q, int32_t width, int32_t levels, int64_t bucket_size,
                             const float* bnorm, float* y_out, int32_t accumulate, void* stream) {
  return sum_bucketed(plan, &q, &bnorm, 1, width, levels, bucket_size, y_out, accumulate, 0.0f, true, stream);
}

int omf_qsgd_decode_sum_bucketed(omf_plan* plan, const void* const* q, const float* const* bnorm, int32_t nclients,
                                 int32_t width, int32_t levels, int64_t bucket_size, float* y_out, int32_t init,
                                 float divisor, void* stream) {
  return sum_bucketed(plan, q, bnorm, nclients, width, levels, bucket_size, y_out, init, divisor, false, stream);
}

int omf_plan_set_bucket_rows(omf_plan* plan, int32_t rows, int32_t static_d) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (rows != 4 && rows != 8 && rows != 16) return fail(OMF_EINVAL, "omf_plan_set_bucket_rows: rows must be 4, 8 or 16");
  plan->bucket_rows = rows;
  plan->bucket_static_d = static_d != 0;
  return OMF_OK;
}

}  // extern "C"
