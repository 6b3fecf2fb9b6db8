// omf_qsgd_bucket_rot.hip — bucketed QSGD with max-norm buckets and a fused randomised Hadamard rotation, MI355X
// (gfx950): the encoder, the transform alone and the K-client decode-and-sum, with their host side.  The rules
// (signs, the butterfly's stage order, the scale) are omf_qsgd_bucket_rot.h; buckets and their arena are
// omf_qsgd_bucket.h's, the draws, the level math and the payload stores the other encoders' (omf_qsgd_enc.h), the
// decode rule and the sums' chaining the other decoders' (omf_qsgd_dec.h).  DESIGN.md §3.4g.
//
// All three kernels share the bucketed encoder's shape: one 256-thread workgroup per block of 4 rows (4096
// elements) of a flat 16 Ki item, row k of thread tid the quad at 4 (k 256 + tid) of the block, blocks a multiple
// of 4096 elements after their tensor's begin — so a bucket is d / 4 consecutive lanes of one row or 2 / 4 of a
// thread's own rows, and a Walsh-Hadamard stage is a DPP / permlane exchange, one LDS tile across the waves, or a
// register pair.  No workgroup waits for another.
//
// Kernel map:
//   qsgd_bucket_encode_max<WIDTH, HAS_U, ROT, LOGD>   x read once (non-temporal) into registers; scale; (ROT) signs
//                    and butterfly on full buckets; the bucket's max |z| (bucket_maxes), stored by the bucket's
//                    first lane; quant_rows against it with store_quad as the sink.  The draws keep philox_rows'
//                    keying: the same seed and offset give the uniforms of qsgd_bucket_encode.  A NULL q stops
//                    after the scales.
//   qsgd_bucket_rotate<LOGD>   the transform alone, forward or inverse, arena to arena; short last buckets are
//                    copied.
//   qsgd_bucket_decode_sum_rot<WIDTH, POW2, N>   N clients' quads decoded (dec_quad) and added in client order in
//                    the rotated domain — the transform is linear, so K clients cost one inverse — then the
//                    inverse, y = init ? y + xh : xh, / divisor, a non-temporal store.  A call of more than 8
//                    clients that does not start from y keeps its running sum in y in the rotated domain between
//                    launches (from_rot / to_rot), so it too is one client-order sum and one inverse; one that
//                    starts from y adds each launch's inverse to y.  The block that ends its tensor fills the
//                    padding behind it (the first block of the arena also the gap in front) under the `fill` rule.
//
// Not HBM-bound; no MFMA (a butterfly of adds has no contraction to feed one).
#include <string>
#include <vector>

#include "../../include/omf_codec.h"
#include "omf_bracket.h"  // EncCall, enc_args, launch_kernel
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_bucket.h"
#include "omf_qsgd_bucket_rot.h"
#include "omf_qsgd_dec.h"
#include "omf_qsgd_enc.h"

using namespace omf;
using namespace omf::plan_layout;

namespace {

// ---------------------------------------------------------------- encoder

template <int WIDTH, bool HAS_U, bool ROT, bool FULL>
__device__ __forceinline__ void max_block(const EncArgs& a, const RotGeom& g, const Blk& bk, int logd, float4* tile,
                                          uint32_t (*xch)[kWaves]) {
  const int tid = (int)threadIdx.x;
  float4 v[kRows];
  load_f4<kRows, FULL, true>(a.x, bk.b, bk.end, v);  // read once: non-temporal
  scale_f4<kRows>(v, a);
  float z[kRows][4];
#pragma unroll
  for (int k = 0; k < kRows; ++k) { z[k][0] = v[k].x; z[k][1] = v[k].y; z[k][2] = v[k].z; z[k][3] = v[k].w; }
  if (ROT) rotate_block<false, FULL>(z, g, bk, logd, tile);
  // the scales: computed, or the caller's
  const int64_t nbase = g.boff[bk.tensor];
  float norm[kRows];
  if (a.norm_in) {  // uniform
    bucket_norms_in<FULL, kRows>(a.norm_in, bk.b, bk.end, bk.tbegin, nbase, logd, norm);
  } else {
    uint32_t m[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const uint32_t abs = 0x7FFFFFFFu;
      m[k] = max(max(__float_as_uint(z[k][0]) & abs, __float_as_uint(z[k][1]) & abs),
                 max(__float_as_uint(z[k][2]) & abs, __float_as_uint(z[k][3]) & abs));
    }
    bucket_rot::bucket_maxes(m, logd, xch);
#pragma unroll
    for (int k = 0; k < kRows; ++k) norm[k] = __uint_as_float(m[k]);
  }
  bucket_norms_store<FULL, kRows>(a.norm_out, bk.b, bk.end, bk.tbegin, nbase, logd, norm);
  if (!a.q) return;  // scales only (uniform)
#pragma unroll
  for (int k = 0; k < kRows; ++k) v[k] = make_float4(z[k][0], z[k][1], z[k][2], z[k][3]);
  quant_rows<HAS_U, FULL, kRows>(v, a, bk.b, bk.end, bk.tbegin, bk.tensor, norm,
                                 [&](int, int64_t e, const int32_t (&qq)[4]) { store_quad<WIDTH, FULL>(a, e, bk.end, qq); });
}

template <int WIDTH, bool HAS_U, bool ROT, int LOGD>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_encode_max(EncArgs a, RotGeom g) {
  __shared__ float4 tile[(ROT && LOGD >= 9) ? bucket_rot::kTileQuads : 1];
  __shared__ uint32_t xch[kRows][kWaves];
  const Blk bk = block_of(g);
  if (bk.b >= bk.end) return;
  if (bk.end - bk.b == kBlk) max_block<WIDTH, HAS_U, ROT, true>(a, g, bk, LOGD, tile, xch);
  else max_block<WIDTH, HAS_U, ROT, false>(a, g, bk, LOGD, tile, xch);
}

using MaxKernel = void (*)(EncArgs, RotGeom);

template <int LOGD>
MaxKernel encode_kernel(bool int32_wire, bool has_u, bool rot) {
  static const MaxKernel kern[2][2][2] = {
      {{qsgd_bucket_encode_max<1, false, false, LOGD>, qsgd_bucket_encode_max<1, false, true, LOGD>},
       {qsgd_bucket_encode_max<1, true, false, LOGD>, qsgd_bucket_encode_max<1, true, true, LOGD>}},
      {{qsgd_bucket_encode_max<4, false, false, LOGD>, qsgd_bucket_encode_max<4, false, true, LOGD>},
       {qsgd_bucket_encode_max<4, true, false, LOGD>, qsgd_bucket_encode_max<4, true, true, LOGD>}}};
  return kern[int32_wire][has_u][rot];
}

// f(std::integral_constant<int, logd>) for logd = 6 .. 12.
template <class F>
void with_logd(int logd, F&& f) {
  switch (logd) {
#define OMF_L(L) case L: f(std::integral_constant<int, L>{}); break;
    OMF_L(6) OMF_L(7) OMF_L(8) OMF_L(9) OMF_L(10) OMF_L(11)
#undef OMF_L
    default: f(std::integral_constant<int, 12>{}); break;
  }
}

// ---------------------------------------------------------------- the transform alone

template <bool INVERSE, bool FULL>
__device__ __forceinline__ void rotate_rows(const float* x, float* y, const RotGeom& g, const Blk& bk, int logd,
                                            float4* tile) {
  float4 v[kRows];
  load_f4<kRows, FULL, true>(x, bk.b, bk.end, v);
  float z[kRows][4];
#pragma unroll
  for (int k = 0; k < kRows; ++k) { z[k][0] = v[k].x; z[k][1] = v[k].y; z[k][2] = v[k].z; z[k][3] = v[k].w; }
  rotate_block<INVERSE, FULL>(z, g, bk, logd, tile);
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = bk.b + 4 * ((int64_t)k * kThreads + threadIdx.x);
    if (FULL || e < bk.end) store_f4<FULL>(y, e, bk.end, z[k]);
  }
}

template <int LOGD>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_rotate(const float* __restrict__ x, float* __restrict__ y,
                                                               RotGeom g, int inverse) {
  __shared__ float4 tile[LOGD >= 9 ? bucket_rot::kTileQuads : 1];
  const Blk bk = block_of(g);
  if (bk.b >= bk.end) return;
  const bool full = bk.end - bk.b == kBlk;
  if (inverse) {
    if (full) rotate_rows<true, true>(x, y, g, bk, LOGD, tile);
    else rotate_rows<true, false>(x, y, g, bk, LOGD, tile);
  } else {
    if (full) rotate_rows<false, true>(x, y, g, bk, LOGD, tile);
    else rotate_rows<false, false>(x, y, g, bk, LOGD, tile);
  }
}

// ---------------------------------------------------------------- decode and sum

struct RotSum {
  int32_t from_rot;  // the sum starts from y, a running sum in the rotated domain
  int32_t to_rot;    // the sum is stored as it is: no inverse, no y, no divisor
};

template <int WIDTH, bool POW2, int N, bool FULL>
__device__ __forceinline__ void sum_block(const BSumArgs<N>& a, const RotGeom& g, const RotSum& r, const Blk& bk,
                                          float4* tile) {
  const int tid = (int)threadIdx.x, logd = g.logd;
  const int64_t rel = (bk.b - bk.tbegin) + 4 * tid, nbase = g.boff[bk.tensor];
  float z[kRows][4];
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = bk.b + 4 * ((int64_t)k * kThreads + tid);
    const float4 s0 = r.from_rot ? load_quad<FULL, true>(a.y, e, bk.end) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    z[k][0] = s0.x; z[k][1] = s0.y; z[k][2] = s0.z; z[k][3] = s0.w;
  }
#pragma unroll
  for (int c = 0; c < N; ++c) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const int64_t e = bk.b + 4 * ((int64_t)k * kThreads + tid);
      const bool live = FULL || e < bk.end;
      int32_t rr[4];
      load_levels<WIDTH, FULL>(a.q[c], e, bk.end, rr);
      const float m = live ? a.norm[c][nbase + ((rel + 1024 * k) >> logd)] : 0.0f;
      float yv[4];
      dec_quad<WIDTH, POW2>(rr, m, a.levels, a.inv_levels, yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) z[k][j] = live ? __fadd_rn(z[k][j], yv[j]) : 0.0f;
    }
  }
  if (!r.to_rot) {
    rotate_block<true, FULL>(z, g, bk, logd, tile);
    if (a.init) {
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        const float4 p = load_quad<FULL, true>(a.y, bk.b + 4 * ((int64_t)k * kThreads + tid), bk.end);
        z[k][0] = __fadd_rn(p.x, z[k][0]); z[k][1] = __fadd_rn(p.y, z[k][1]);
        z[k][2] = __fadd_rn(p.z, z[k][2]); z[k][3] = __fadd_rn(p.w, z[k][3]);
      }
    }
    if (a.divisor != 0.0f) {
#pragma unroll
      for (int k = 0; k < kRows; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) z[k][j] = z[k][j] / a.divisor;
    }
  }
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = bk.b + 4 * ((int64_t)k * kThreads + tid);
    if (FULL || e < bk.end) store_f4<FULL>(a.y, e, bk.end, z[k]);
  }
}

template <int WIDTH, bool POW2, int N>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_decode_sum_rot(BSumArgs<N> a, RotGeom g, RotSum r) {
  __shared__ float4 tile[bucket_rot::kTileQuads];
  const Blk bk = block_of(g);
  if (bk.b >= bk.end) return;
  if (bk.end - bk.b == kBlk) sum_block<WIDTH, POW2, N, true>(a, g, r, bk, tile);
  else sum_block<WIDTH, POW2, N, false>(a, g, r, bk, tile);
  if (!a.fill) return;
  // the padding of [0, arena_end): behind the tensor this block ends, and in front of the arena's first tensor
  const float pad = a.pad_div != 0.0f ? 0.0f / a.pad_div : 0.0f;
  if (bk.end == bk.tbegin + bk.tn) {
    const int64_t stop = bk.tensor + 1 < g.nt ? min(g.begins[bk.tensor + 1], g.arena_end) : g.arena_end;
    for (int64_t i = bk.end + threadIdx.x; i < stop; i += kThreads) a.y[i] = pad;
  }
  if (bk.tensor == 0 && bk.b == bk.tbegin) {
    for (int64_t i = threadIdx.x; i < min(bk.tbegin, g.arena_end); i += kThreads) a.y[i] = pad;
  }
}

// ---------------------------------------------------------------- host side

int encode_max(omf_plan* p, const float* x, float alpha, int32_t s, int64_t d, const float* u, uint64_t seed,
               uint64_t offset, const float* bnorm_in, void* q, float* bnorm_out, bool rotate, uint32_t rot_seed,
               int32_t tensor_keyed, bool norm_only, void* stream) {
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
  DeviceGuard dg(p->device);
  if (!dg.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  RotGeom g;
  if (int r = rot_geom(p, logd, rot_seed, tensor_keyed, &g)) return r;
  const hipStream_t st = (hipStream_t)stream;
  EncArgs a = enc_args(p, EncCall{x, alpha, s, u, seed, offset, bnorm_in, norm_only ? nullptr : q, bnorm_out, norm_only,
                                  st, 0.0f, nullptr, 0u, nullptr, width});
  with_logd(logd, [&](auto L) {
    launch_kernel(encode_kernel<L()>(width == 4, u != nullptr, rotate), dim3(rot_grid_blocks(p)), dim3(kThreads), 0, st, a, g);
  });
  OMF_HIP(hipGetLastError());
  if (!norm_only) p->last_encoder = rotate ? kEncBucketedMaxRot : kEncBucketedMax;
  return OMF_OK;
}

int rotate_bucketed(omf_plan* p, const float* x, int64_t d, uint32_t rot_seed, int32_t tensor_keyed, int32_t inverse, float* y,
                    void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd = bucket::log2_size(d);
  if (logd < 0) return fail(OMF_EINVAL, kBucketBadSize);
  if (!x || !y) return fail(OMF_EINVAL, "x and y_out must be non-NULL");
  if (!aligned(x, 16) || !aligned(y, 16)) return fail(OMF_EINVAL, kBucketMisaligned);
  const size_t bytes = (size_t)p->arena_end * 4;
  if (x != y && overlaps(y, bytes, x, bytes)) return fail(OMF_EINVAL, "omf_qsgd_rotate_bucketed: y_out overlaps x (y_out == x is in place)");
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  DeviceGuard dg(p->device);
  if (!dg.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  RotGeom g;
  if (int r = rot_geom(p, logd, rot_seed, tensor_keyed, &g)) return r;
  const int inv = inverse != 0;
  with_logd(logd, [&](auto L) {
    hipLaunchKernelGGL((qsgd_bucket_rotate<L()>), dim3(rot_grid_blocks(p)), dim3(kThreads), 0, (hipStream_t)stream, x, y, g, inv);
  });
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}

// omf_qsgd_bucketed.hip's sum_bucketed with the rotation's arguments: the same checks (bucket_sum_checks), then the
// chained groups.
int sum_rot(omf_plan* p, const void* const* q, const float* const* bnorm, int32_t nclients, int32_t width, int32_t levels,
            int64_t d, uint32_t rot_seed, int32_t tensor_keyed, float* y, int32_t init, float divisor, bool plain, void* stream) {
  const std::string who = plain ? "omf_qsgd_decode_bucketed_rot" : "omf_qsgd_decode_sum_bucketed_rot";
  int logd = 0;
  if (int r = bucket_sum_checks(p, q, bnorm, nclients, width, levels, d, y, plain, who, &logd)) return r;
  DeviceGuard dg(p->device);
  if (!dg.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  RotGeom g;
  if (int r = rot_geom(p, logd, rot_seed, tensor_keyed, &g)) return r;
  const LevelScale lv(levels);
  SumCallBase c;
  c.y = y; c.st = (hipStream_t)stream; c.levels = lv.levels; c.inv_levels = lv.inv_levels;
  const bool chain_rot = !init && nclients > kBucketSumMax;  // the running sum lives in y, in the rotated domain
  for (int32_t k0 = 0; k0 < nclients; k0 += kBucketSumMax) {
    c.g = sum_group(nclients, kBucketSumMax, init, divisor, k0);
    if (plain) c.g.fill = 0;
    c.norm = bnorm + k0;
    RotSum r{0, 0};
    if (chain_rot) {
      r.from_rot = k0 > 0;
      r.to_rot = k0 + c.g.n < nclients;
      c.g.init = 0;
    }
    with_group_size<kBucketSumMax>(c.g.n, [&](auto N) {
      BSumArgs<N()> a{};
      for (int k = 0; k < N(); ++k) a.q[k] = q[k0 + k];
      sum_common_args(a, c, N());
      auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(rot_grid_blocks(p)), dim3(kThreads), 0, c.st, a, g, r); };
      if (width == 8) {
        if (lv.pow2) go(qsgd_bucket_decode_sum_rot<1, true, N()>); else go(qsgd_bucket_decode_sum_rot<1, false, N()>);
      } else {
        if (lv.pow2) go(qsgd_bucket_decode_sum_rot<4, true, N()>); else go(qsgd_bucket_decode_sum_rot<4, false, N()>);
      }
    });
    OMF_HIP(hipGetLastError());
  }
  return OMF_OK;
}

}  // namespace

extern "C" {

int omf_qsgd_encode_bucketed_max(omf_plan* plan, const float* x, float alpha, int32_t bit_width, int64_t bucket_size,
                                 const float* u, uint64_t seed, uint64_t offset, const float* bnorm_in, void* q_out,
                                 float* bnorm_out, int32_t rotate, uint32_t rot_seed, int32_t tensor_keyed,
                                 void* stream) {
  return encode_max(plan, x, alpha, bit_width, bucket_size, u, seed, offset, bnorm_in, q_out, bnorm_out, rotate != 0,
                    rot_seed, tensor_keyed, false, stream);
}

int omf_qsgd_scales_bucketed_max(omf_plan* plan, const float* x, float alpha, int64_t bucket_size, int32_t rotate,
                                 uint32_t rot_seed, int32_t tensor_keyed, float* bnorm_out, void* stream) {
  return encode_max(plan, x, alpha, 0, bucket_size, nullptr, 0, 0, nullptr, nullptr, bnorm_out, rotate != 0, rot_seed,
                    tensor_keyed, true, stream);
}

int omf_qsgd_rotate_bucketed(omf_plan* plan, const float* x, int64_t bucket_size, uint32_t rot_seed, int32_t tensor_keyed,
                             int32_t inverse, float* y_out, void* stream) {
  return rotate_bucketed(plan, x, bucket_size, rot_seed, tensor_keyed, inverse, y_out, stream);
}

int omf_qsgd_decode_bucketed_rot(omf_plan* plan, const void* q, int32_t width, int32_t levels, int64_t bucket_size,
                                 uint32_t rot_seed, int32_t tensor_keyed, const float* bnorm, float* y_out,
                                 int32_t accumulate, void* stream) {
  return sum_rot(plan, &q, &bnorm, 1, width, levels, bucket_size, rot_seed, tensor_keyed, y_out, accumulate, 0.0f, true, stream);
}

int omf_qsgd_decode_sum_bucketed_rot(omf_plan* plan, const void* const* q, const float* const* bnorm, int32_t nclients,
                                     int32_t width, int32_t levels, int64_t bucket_size, uint32_t rot_seed, int32_t tensor_keyed,
                                     float* y_out, int32_t init, float divisor, void* stream) {
  return sum_rot(plan, q, bnorm, nclients, width, levels, bucket_size, rot_seed, tensor_keyed, y_out, init, divisor, false, stream);
}

int omf_qsgd_rotation_signs(uint32_t rot_seed, int32_t tensor, int64_t begin, int64_t count, int8_t* signs_out) {
  if (tensor < 0 || begin < 0 || count < 0) return fail(OMF_EINVAL, "omf_qsgd_rotation_signs: tensor, begin and count must be >= 0");
  if (count && !signs_out) return fail(OMF_EINVAL, "omf_qsgd_rotation_signs: signs_out is NULL");
  bucket_rot::signs(rot_seed, (uint32_t)tensor, begin, count, signs_out);
  return OMF_OK;
}

}  // extern "C"
