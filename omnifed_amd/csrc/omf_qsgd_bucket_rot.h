// omf_qsgd_bucket_rot.h — the rules of max-scaled bucketed QSGD and its randomised Hadamard rotation
// (omf_qsgd_bucket_rot.hip), one copy of each.  Not part of the C ABI.  The host rules come first and are plain
// C++ with no HIP header; the device rules follow under __HIPCC__.
//
// Buckets, their arena and d are omf_qsgd_bucket.h's.  What differs is the scale of a bucket and, opt-in, the
// domain its levels are taken in (Suresh et al., 2017, "rotated uniform quantisation"):
//   v        fl32(alpha x), as every encoder forms it;
//   sigma_j  +1 or -1 for element j of tensor t: bit (j & 31) of sign_word(rot_seed, t, j >> 5), set = -1.  A
//            stateless integer mix (the murmur3 finaliser, twice): no table, no memory traffic, the same inline
//            function on host and device.  A call with tensor_keyed = 0 takes t = 0 for every tensor (the hybrid
//            wire: a layer then inverts in any plan);
//   z        a FULL bucket of d = 2^logd elements with rotation on: z = H_d (sigma . v), the unnormalised
//            Walsh-Hadamard transform, fp32 adds and subtracts only (no fma), one butterfly stage per bit of the
//            element's index within the bucket, in ascending order of that bit.  Stage `bit` maps the pair
//            (a, b) = (element with the bit clear, element with it set) to (a + b, a - b).  The order is fixed, so
//            z's bits depend only on the bucket's values, sigma and d.  A tensor's short last bucket (every
//            tensor shorter than d is one) is never rotated: z = v.  So is every bucket with rotation off;
//   m        the bucket's scale: max |z_i|, absent elements of a short bucket taken as +0.  A max has no rounding
//            and no order; it is taken on the bit patterns of |z_i| as unsigned integers, which order finite
//            values as their magnitudes do and put +inf above them and every NaN above +inf;
//   levels   qsgd_quad of z against Divisor(m): |level| <= L.  m = 0 gives zero levels, as a zero norm does;
//   decode   zh = fl32(fl32(m q) / L), the wire's rule unchanged; a rotated bucket's values are
//            xh = sigma . (H_d zh) 2^-logd with the same butterfly; the scaling by 2^-logd is exact wherever
//            the result is a normal number (it rounds once where it is subnormal).
// Overflow: |z_i| <= sum |v_j|, so the forward transform overflows only for |v| > FLT_MAX / d.
// Non-finite elements: a NaN or an infinity in a bucket makes that bucket's scale non-finite (NaN wins over inf;
// with rotation on, inf - inf of the butterfly may make it NaN): the bucket's levels are then unspecified and
// every element of it decodes to a non-finite value or zero.  No exchange below crosses a bucket's boundary with a
// value that is kept, so no other bucket is affected.
//
// Where the stages run (a workgroup's block of 4 rows, row k of thread tid the quad at 4 (k 256 + tid) of the
// block, blocks a multiple of 4096 elements after their tensor's begin — the bucketed encoder's shape):
//   bits 0-1    inside the lane's quad;
//   bits 2-5    DPP inside a row of 16 lanes (lane ^ 1, 2, 4, 8: bucket::lane_group_sum's controls);
//   bits 6, 7   v_permlane16_swap, v_permlane32_swap;
//   bits 8-9    across the four waves through one LDS tile: one radix-4 exchange, one barrier, 16 KiB;
//   bits 10-11  between the thread's own rows k ^ 1 and k ^ 2.
// Only stages below logd run: from d <= 256 there is no LDS traffic and no barrier.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "omf_qsgd_bucket.h"

#ifdef __HIPCC__
#define OMF_ROT_HD __host__ __device__ __forceinline__
#else
#define OMF_ROT_HD inline
#endif

namespace omf {
namespace bucket_rot {

// ---------------------------------------------------------------- host rules (sign_word: host and device)

OMF_ROT_HD uint32_t fmix32(uint32_t h) {  // murmur3's finaliser: a bijection of 32-bit words
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

// The signs of elements 32 w .. 32 w + 31 of tensor `tensor`.
OMF_ROT_HD uint32_t sign_word(uint32_t rot_seed, uint32_t tensor, uint64_t w) {
  const uint32_t h = fmix32(rot_seed + 0x9E3779B1u * (tensor + 1u));
  return fmix32(h ^ (uint32_t)w ^ ((uint32_t)(w >> 32) * 0xC2B2AE3Du));
}

// out[i] = sigma of element begin + i of the tensor, i < count, as +1 / -1 bytes.
inline void signs(uint32_t rot_seed, uint32_t tensor, int64_t begin, int64_t count, int8_t* out) {
  for (int64_t i = 0; i < count; ++i) {
    const int64_t j = begin + i;
    out[i] = (sign_word(rot_seed, tensor, (uint64_t)j >> 5) >> (j & 31)) & 1u ? -1 : 1;
  }
}

}  // namespace bucket_rot
}  // namespace omf

#ifdef __HIPCC__

namespace omf {
namespace bucket_rot {

// ---------------------------------------------------------------- device rules

constexpr int kRows = 4;                       // rows of 1024 elements per workgroup
constexpr int kBlk = kRows * 4 * kThreads;     // 4096: the largest bucket
constexpr int kTileQuads = kRows * kThreads;   // the wave exchange's LDS tile, in float4 (16 KiB)

// One stage between this lane's value and its partner's: the lane whose index bit is clear keeps a + b, the
// other a - b.
__device__ __forceinline__ float bfly(float own, float partner, bool hi) {
  return hi ? __fsub_rn(partner, own) : __fadd_rn(own, partner);
}

// sigma applied to the quad at element `rel` (a multiple of 4) of tensor `tensor`, in place.
__device__ __forceinline__ void apply_signs(float (&z)[4], uint32_t rot_seed, int32_t tensor, int64_t rel) {
  const uint32_t bits = sign_word(rot_seed, (uint32_t)tensor, (uint64_t)rel >> 5) >> ((uint32_t)rel & 31u);
#pragma unroll
  for (int c = 0; c < 4; ++c) z[c] = __uint_as_float(__float_as_uint(z[c]) ^ (((bits >> c) & 1u) << 31));
}

// The stage of a swap instruction of a value with itself: r0 is the value of the lane whose index bit is clear,
// r1 of the lane whose bit is set, in both lanes of the pair (bucket::lane_group_sum) — so the lane's half says
// which result is its partner's.
__device__ __forceinline__ float swap_stage(float own, uint32_t r0, uint32_t r1, bool hi) {
  return bfly(own, __uint_as_float(hi ? r0 : r1), hi);
}

// H_d over the buckets of a block, in place: z[k] is this thread's quad of row k.  Called by the whole
// workgroup with every lane active (lanes past the block's end hold +0); logd is uniform.  tile: kTileQuads
// float4 of LDS, touched only from d = 512 up.
__device__ __forceinline__ void wht_rows(float (&z)[kRows][4], int logd, float4* tile) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {  // bits 0, 1
    const float a = __fadd_rn(z[k][0], z[k][1]), b = __fsub_rn(z[k][0], z[k][1]);
    const float c = __fadd_rn(z[k][2], z[k][3]), d = __fsub_rn(z[k][2], z[k][3]);
    z[k][0] = __fadd_rn(a, c); z[k][1] = __fadd_rn(b, d);
    z[k][2] = __fsub_rn(a, c); z[k][3] = __fsub_rn(b, d);
  }
#pragma unroll
  for (int k = 0; k < kRows; ++k) {  // bits 2 .. 5: d >= 64
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float s = z[k][c];
      s = bfly(s, bucket::dpp_f32<0xB1>(s), tid & 1);                       // lane ^ 1
      s = bfly(s, bucket::dpp_f32<0x4E>(s), tid & 2);                       // lane ^ 2
      s = bfly(s, bucket::dpp_f32<0x1B>(bucket::dpp_f32<0x141>(s)), tid & 4);  // lane ^ 4
      s = bfly(s, bucket::dpp_f32<0x128>(s), tid & 8);                      // lane ^ 8
      if (logd >= 7) {
        const uint32_t b = __float_as_uint(s);
        const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
        s = swap_stage(s, r[0], r[1], tid & 16);
      }
      if (logd >= 8) {
        const uint32_t b = __float_as_uint(s);
        const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
        s = swap_stage(s, r[0], r[1], tid & 32);
      }
      z[k][c] = s;
    }
  }
  if (logd >= 9) {  // bits 8, 9: the waves
#pragma unroll
    for (int k = 0; k < kRows; ++k) tile[k * kThreads + tid] = make_float4(z[k][0], z[k][1], z[k][2], z[k][3]);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      if (logd == 9) {
        const float4 p = tile[k * kThreads + (tid ^ 64)];
        const float pp[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) z[k][c] = bfly(z[k][c], pp[c], wave & 1);
      } else {
        float q[4][4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const float4 p = tile[k * kThreads + w * 64 + lane];
          q[w][0] = p.x; q[w][1] = p.y; q[w][2] = p.z; q[w][3] = p.w;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // bit 8: (w0, w1), (w2, w3); bit 9: their results two waves apart
          const float lo = (wave & 1) ? __fsub_rn(q[0][c], q[1][c]) : __fadd_rn(q[0][c], q[1][c]);
          const float hi = (wave & 1) ? __fsub_rn(q[2][c], q[3][c]) : __fadd_rn(q[2][c], q[3][c]);
          z[k][c] = (wave & 2) ? __fsub_rn(lo, hi) : __fadd_rn(lo, hi);
        }
      }
    }
  }
  if (logd >= 11) {  // bit 10: rows k ^ 1
#pragma unroll
    for (int k = 0; k < kRows; k += 2) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float a = z[k][c], b = z[k + 1][c];
        z[k][c] = __fadd_rn(a, b); z[k + 1][c] = __fsub_rn(a, b);
      }
    }
  }
  if (logd >= 12) {  // bit 11: rows k ^ 2
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float a = z[k][c], b = z[k + 2][c];
        z[k][c] = __fadd_rn(a, b); z[k + 2][c] = __fsub_rn(a, b);
      }
    }
  }
}

// bucket::bucket_sums with max in place of add, on the bit patterns of |z|: m[k] enters as the max over this
// thread's quad of row k and leaves as the max over the bucket that holds it.  xch: kRows x kWaves words of
// LDS, one exchange (one barrier) from d = 512 up; called by the whole workgroup.
__device__ __forceinline__ void bucket_maxes(uint32_t (&m)[kRows], int logd, uint32_t (*xch)[kWaves]) {
  if (logd >= 11) {
#pragma unroll
    for (int k = 0; k < kRows; k += 2) m[k] = m[k + 1] = max(m[k], m[k + 1]);
  }
  if (logd >= 12) m[0] = m[1] = m[2] = m[3] = max(m[0], m[2]);
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    uint32_t s = m[k];
    s = max(s, dpp_mov<0xB1>(s));
    s = max(s, dpp_mov<0x4E>(s));
    s = max(s, dpp_mov<0x1B>(dpp_mov<0x141>(s)));
    s = max(s, dpp_mov<0x128>(s));
    if (logd >= 7) {
      const auto r = __builtin_amdgcn_permlane16_swap(s, s, false, false);
      s = max(r[0], r[1]);
    }
    if (logd >= 8) {
      const auto r = __builtin_amdgcn_permlane32_swap(s, s, false, false);
      s = max(r[0], r[1]);
    }
    m[k] = s;
  }
  if (logd < 9) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) xch[k][wave] = m[k];
  }
  __syncthreads();
  const int w0 = wave & 2;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    if (logd == 9) m[k] = max(xch[k][w0], xch[k][w0 + 1]);
    else m[k] = max(max(xch[k][0], xch[k][1]), max(xch[k][2], xch[k][3]));
  }
}

}  // namespace bucket_rot
}  // namespace omf

// ---------------------------------------------------------------- what the rotation's units share
// (omf_qsgd_bucket_rot.hip: the encoder, the transform and the sums; omf_qsgd_bucket_ps_max.hip: the PS step over
// them).  In an unnamed namespace, as the bucketed units' shared steps are (omf_qsgd_bucket.h).

namespace {

using namespace omf;
using namespace omf::plan_layout;
using bucket_rot::kBlk;
using bucket_rot::kRows;

// What every kernel of these units takes from the plan and the call.
struct RotGeom {
  const Item* items;      // the plan's flat items
  const int64_t* begins;  // per tensor
  const int64_t* sizes;
  const int64_t* boff;    // the tensors' offsets into the bucket arena at this d
  int64_t arena_end;
  int32_t nt;
  uint32_t rot_seed;
  int32_t tensor_mask;    // -1: sigma keyed by the plan's tensor index; 0: by the element alone (every tensor as tensor 0)
  int32_t logd;
};

// This workgroup's block [b, end) of tensor `tensor` ([tbegin, tbegin + tn)); b >= end: none.
struct Blk {
  int64_t b, end, tbegin, tn;
  int32_t tensor;
};
__device__ __forceinline__ Blk block_of(const RotGeom& g) {
  constexpr int PER = (int)(kSub / kBlk);
  const Item it = g.items[blockIdx.x / PER];
  Blk k;
  k.b = it.begin + (int64_t)(blockIdx.x % PER) * kBlk;
  k.end = min(k.b + (int64_t)kBlk, it.end);
  k.tensor = it.tensor;
  k.tbegin = g.begins[it.tensor];
  k.tn = g.sizes[it.tensor];
  return k;
}

// The transform of a block's rows in place, forward (z = H (sigma . v)) or inverse (xh = sigma . (H zh) 2^-logd),
// on the quads of full buckets; the others keep their values.  A FULL block holds full buckets only (d divides
// 4096).  Called by the whole workgroup, lanes past `end` holding +0: in a mixed block every lane runs the
// exchanges.
template <bool INVERSE, bool FULL>
__device__ __forceinline__ void rotate_block(float (&z)[kRows][4], const RotGeom& g, const Blk& bk, int logd,
                                             float4* tile) {
  const int64_t rel = (bk.b - bk.tbegin) + 4 * (int)threadIdx.x;  // this thread's row 0, from the tensor's begin
  float keep[kRows][4];
  if (!FULL) {
#pragma unroll
    for (int k = 0; k < kRows; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) keep[k][c] = z[k][c];
  }
  if (!INVERSE) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) bucket_rot::apply_signs(z[k], g.rot_seed, bk.tensor & g.tensor_mask, rel + 1024 * k);
  }
  bucket_rot::wht_rows(z, logd, tile);
  if (INVERSE) {
    const float inv_d = __uint_as_float((uint32_t)(127 - logd) << 23);  // 2^-logd
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
#pragma unroll
      for (int c = 0; c < 4; ++c) z[k][c] = __fmul_rn(z[k][c], inv_d);
      bucket_rot::apply_signs(z[k], g.rot_seed, bk.tensor & g.tensor_mask, rel + 1024 * k);
    }
  }
  if (!FULL) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const bool full = ((((rel + 1024 * k) >> logd) + 1) << logd) <= bk.tn;
#pragma unroll
      for (int c = 0; c < 4; ++c) z[k][c] = full ? z[k][c] : keep[k][c];
    }
  }
}

// A live quad's (e < end) floats out: one non-temporal 16-byte store when whole, else its elements one by one.
template <bool FULL>
__device__ __forceinline__ void store_f4(float* y, int64_t e, int64_t end, const float (&f)[4]) {
  if (FULL || e + 4 <= end) {
    store_nt(y + e, make_float4(f[0], f[1], f[2], f[3]));
  } else {
    y[e] = f[0];
    if (e + 1 < end) y[e + 1] = f[1];
    if (e + 2 < end) y[e + 2] = f[2];
  }
}

// The levels of the quad at e of a payload whose tensor ends at `end`: raw[0] (WIDTH 1: the dword of four int8)
// or raw[0..3]; a partial last quad element by element (the payload may end with it), zeros past the end.
template <int WIDTH, bool FULL>
__device__ __forceinline__ void load_levels(const void* q, int64_t e, int64_t end, int32_t (&rr)[4]) {
  rr[0] = rr[1] = rr[2] = rr[3] = 0;
  if (FULL || e + 4 <= end) {
    if (WIDTH == 1) {
      rr[0] = __builtin_nontemporal_load(reinterpret_cast<const int32_t*>(reinterpret_cast<const int8_t*>(q) + e));
    } else {
      const i32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(reinterpret_cast<const int32_t*>(q) + e));
      rr[0] = t[0]; rr[1] = t[1]; rr[2] = t[2]; rr[3] = t[3];
    }
  } else if (e < end) {
    qsgd_last_quad<WIDTH>(q, e, end, rr);
  }
}

// The kernels' geometry of a call at bucket size 2^logd (the plan's table of that size is made at the first one).
inline int rot_geom(omf_plan* p, int logd, uint32_t rot_seed, int32_t tensor_keyed, RotGeom* g) {
  int64_t nb = 0;
  if (int r = bucket_tables(p, logd, &g->boff, &nb)) return r;
  g->items = p->d_flat;
  g->begins = p->d_begins;
  g->sizes = p->d_sizes;
  g->arena_end = p->arena_end;
  g->nt = p->nt;
  g->rot_seed = rot_seed;
  g->tensor_mask = tensor_keyed ? -1 : 0;
  g->logd = logd;
  return OMF_OK;
}

// One workgroup per block of every flat item.
inline unsigned rot_grid_blocks(const omf_plan* p) { return (unsigned)(p->n_flat * (kSub / kBlk)); }

}  // namespace
#endif  // __HIPCC__
