// omf_qsgd_bucket.h — the rules of bucketed QSGD (omf_qsgd_bucketed.hip, omf_qsgd_bucket_pack.hip, omf_qsgd_bucket_ps.hip,
// omf_qsgd_bucket_h16.hip), one copy of each.  Not part of the
// C ABI.  The host rules come first and are plain C++ with no HIP header; the device rules follow under
// __HIPCC__.
//
// Bucketed QSGD quantises consecutive groups of d elements of a tensor, each against its own L2 norm
// (Alistarh et al., QSGD, §3.3: the variance bound min(n / L^2, sqrt(n) / L) holds per bucket, with n = d).
//   d            a power of two in {64, 128, ..., 4096};
//   bucket j     of tensor t is elements [j d, min((j + 1) d, n_t)) of the tensor's flat order: buckets
//                restart at every tensor, the last one may be short;
//   nb_t         ceil(n_t / d) buckets;
//   boff[t]      sum of nb_u over u < t: where tensor t's norms start in a plan's bucket-norm arena, which
//                holds nb = sum of nb_t fp32 norms.
// Per bucket the semantics are the per-tensor ones on the bucket's elements: v = fl32(alpha x),
// norm_b = fl32(sqrt(sum v^2)) in fp32, levels from qsgd_quad with Divisor(norm_b), zero levels for a zero
// norm, decode fl32(fl32(norm_b q) / L).
//
// The summation order of a bucket's sum of squares (fp32 throughout, no contraction other than the fma chain
// written here) is fixed, so a bucket's norm bits depend only on its values and on d — not on the arena
// offset, the plan, the workgroup's size or the run.  With the bucket's elements numbered from its begin and
// absent elements of a short last bucket taken as +0 (adding +0 to a sum of squares changes no bit):
//   1. quad sums      s_i = fma(v3, v3, fma(v2, v2, fma(v1, v1, fma(v0, v0, +0)))) over elements 4i .. 4i + 3;
//   2. rows           d > 1024 only: quad i of the bucket's row r is i = 256 r + lane; the rows' sums of one
//                     lane are added pairwise, r ^ 1 and then (d = 4096) r ^ 2;
//   3. lanes          a butterfly over the quads (or lane sums) of a row: s += s[lane ^ o] for o = 1, 2, 4, 8,
//                     then 16 (d >= 128) and 32 (d >= 256): after it every lane of the bucket's aligned group
//                     of min(d / 4, 64) lanes holds the same bits (fp32 + commutes exactly);
//   4. waves          d >= 512: the groups of 64 lanes are added as w ^ 1 (d = 512: (g0 + g1)), then w ^ 2
//                     (d >= 1024: ((g0 + g1) + (g2 + g3)));
//   5. norm_b = sqrtf(sum), correctly rounded.
// Plain IEEE fp32 with gradual underflow (the build keeps denormals).  oracle/qsgd_bucket.py is the executable form
// of steps 1-5; tests/test_gpu_qsgd_bucket_matrix.py holds every unit's norm bits to it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace omf {
namespace bucket {

// ---------------------------------------------------------------- host rules

constexpr int kMinLog2 = 6, kMaxLog2 = 12;         // d = 64 .. 4096
constexpr int kSizes = kMaxLog2 - kMinLog2 + 1;    // the allowed sizes (a plan caches one table each)

// log2 d of an allowed bucket size, else -1.
inline int log2_size(int64_t d) {
  for (int l = kMinLog2; l <= kMaxLog2; ++l)
    if (d == ((int64_t)1 << l)) return l;
  return -1;
}

// nb_t of a tensor of n > 0 elements.
inline int64_t count(int64_t n, int logd) { return (n + (((int64_t)1 << logd) - 1)) >> logd; }

// boff[0 .. nt) of the tensors' sizes; returns nb.
inline int64_t offsets(const int64_t* sizes, int32_t nt, int logd, int64_t* boff) {
  int64_t nb = 0;
  for (int32_t t = 0; t < nt; ++t) {
    if (boff) boff[t] = nb;
    nb += count(sizes[t], logd);
  }
  return nb;
}

}  // namespace bucket
}  // namespace omf

#ifdef __HIPCC__
#include <string>
#include <vector>

#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_dec.h"
#include "omf_qsgd_enc.h"

namespace omf {
namespace bucket {

// ---------------------------------------------------------------- device rules

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) { return __uint_as_float(dpp_mov<CTRL>(__float_as_uint(v))); }

// Step 3: the butterfly over the aligned group of min(2^(logd - 2), 64) lanes this lane belongs to; every
// lane of the group ends with the group's sum.  logd is wave-uniform (a kernel argument), and every lane of
// the wave must be active.  No LDS traffic: DPP inside a row of 16 lanes, v_permlane16_swap /
// v_permlane32_swap of s with itself across rows (the two results are {own | partner}, as wave_sum_f64).
__device__ __forceinline__ float lane_group_sum(float s, int logd) {
  s = __fadd_rn(s, dpp_f32<0xB1>(s));                   // lane ^ 1: quad_perm [1,0,3,2]
  s = __fadd_rn(s, dpp_f32<0x4E>(s));                   // lane ^ 2: quad_perm [2,3,0,1]
  s = __fadd_rn(s, dpp_f32<0x1B>(dpp_f32<0x141>(s)));   // lane ^ 4: row_half_mirror, then quad_perm [3,2,1,0]
  s = __fadd_rn(s, dpp_f32<0x128>(s));                  // lane ^ 8: row_ror:8
  if (logd >= 7) {
    const uint32_t b = __float_as_uint(s);
    const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    s = __fadd_rn(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  if (logd >= 8) {
    const uint32_t b = __float_as_uint(s);
    const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    s = __fadd_rn(__uint_as_float(r[0]), __uint_as_float(r[1]));
  }
  return s;
}

// Steps 2-4 over a thread's V rows of per-quad sums (step 1's): s[k] becomes the sum of squares of the bucket
// that holds this thread's quad of row k.  Rows are counted from a multiple of 4 rows of the tensor, so the
// rows of one bucket (d > 1024) are k ^ 1 and k ^ 2 in the thread's own registers.  xch: V x kWaves floats of
// LDS, one exchange (one barrier) for every row, only from d = 512 up; called by the whole workgroup.
template <int V>
__device__ __forceinline__ void bucket_sums(float (&s)[V], int logd, float (*xch)[kWaves]) {
  static_assert(V % 4 == 0, "whole buckets of 4096 elements");
  if (logd >= 11) {
#pragma unroll
    for (int k = 0; k < V; k += 2) s[k] = s[k + 1] = __fadd_rn(s[k], s[k + 1]);
  }
  if (logd >= 12) {
#pragma unroll
    for (int k = 0; k < V; k += 4) s[k] = s[k + 1] = s[k + 2] = s[k + 3] = __fadd_rn(s[k], s[k + 2]);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) s[k] = lane_group_sum(s[k], logd);
  if (logd < 9) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) xch[k][wave] = s[k];
  }
  __syncthreads();
  const int w0 = wave & 2;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if (logd == 9) s[k] = __fadd_rn(xch[k][w0], xch[k][w0 + 1]);
    else s[k] = __fadd_rn(__fadd_rn(xch[k][0], xch[k][1]), __fadd_rn(xch[k][2], xch[k][3]));
  }
}

}  // namespace bucket
}  // namespace omf

// ---------------------------------------------------------------- what the bucketed units share
// (omf_qsgd_bucketed.hip: the int8 / int32 wire; omf_qsgd_bucket_pack.hip: the bit-packed wire;
// omf_qsgd_bucket_ps.hip: the PS step over both; omf_qsgd_bucket_h16.hip: both wires from a 16-bit arena).  In an
// unnamed namespace, as the encoders' steps they build on are (omf_qsgd_enc.h).

namespace {

using namespace omf;

constexpr const char* kBucketMisaligned = "misaligned buffer (fp32/int32 need 16 B, int8 needs 4 B alignment)";
constexpr const char* kBucketBadSize = "bucket_size must be a power of two in [64, 4096]";

// The caller's norms (or scales) of a block's V rows: norm[k] of the bucket that holds this thread's quad of row k,
// 0 for a quad past `end`.
template <bool FULL, int V>
__device__ __forceinline__ void bucket_norms_in(const float* __restrict__ norm_in, int64_t b, int64_t end, int64_t tbegin,
                                                int64_t nbase, int logd, float (&norm)[V]) {
  const int tid = (int)threadIdx.x;
  const int64_t rel = (b - tbegin) + 4 * tid;  // this thread's row 0, from the tensor's begin
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const bool live = FULL || b + 4 * ((int64_t)k * kThreads + tid) < end;
    norm[k] = live ? norm_in[nbase + ((rel + 1024 * k) >> logd)] : 0.0f;
  }
}

// The bucket's first lane (of its first row) stores the bucket's norm (or scale).
template <bool FULL, int V>
__device__ __forceinline__ void bucket_norms_store(float* __restrict__ norm_out, int64_t b, int64_t end, int64_t tbegin,
                                                   int64_t nbase, int logd, const float (&norm)[V]) {
  const int tid = (int)threadIdx.x;
  const int64_t rel = (b - tbegin) + 4 * tid;
  const int lane_mask = logd <= 10 ? (1 << (logd - 2)) - 1 : kThreads - 1;
  const int row_mask = logd <= 10 ? 0 : (1 << (logd - 10)) - 1;
  if ((tid & lane_mask) == 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (k & row_mask) continue;
      if (FULL || b + 4 * ((int64_t)k * kThreads + tid) < end) norm_out[nbase + ((rel + 1024 * k) >> logd)] = norm[k];
    }
  }
}

// The norm half of a block's front: v holds the block's V rows of values (+0 at elements past `end`); norm[k]
// becomes the norm of the bucket that holds this thread's quad of row k — computed (bucket_sums) or the
// caller's — and the bucket's first lane (of its first row) stores it.  Called by the whole workgroup.
template <bool FULL, int V>
__device__ __forceinline__ void bucket_norms(const EncArgs& a, int64_t b, int64_t end, int64_t tbegin, int64_t nbase,
                                             int logd, float (*xch)[kWaves], const float4 (&v)[V], float (&norm)[V]) {
  if (a.norm_in) {  // the caller's norms (uniform branch)
    bucket_norms_in<FULL, V>(a.norm_in, b, end, tbegin, nbase, logd, norm);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) norm[k] = sq4(v[k], 0.0f);
    bucket::bucket_sums<V>(norm, logd, xch);
#pragma unroll
    for (int k = 0; k < V; ++k) norm[k] = sqrtf(norm[k]);
  }
  bucket_norms_store<FULL, V>(a.norm_out, b, end, tbegin, nbase, logd, norm);
}

// The front half of one block [b, end) of V rows of a tensor (begins at tbegin; its norms at nbase of the
// bucket arena), the encoders' source: x loaded once (non-temporal) and scaled into v, then bucket_norms.  (The
// PS step's source is K clients' payloads: omf_qsgd_bucket_ps.hip.)
template <bool FULL, int V>
__device__ __forceinline__ void bucket_front(const EncArgs& a, int64_t b, int64_t end, int64_t tbegin, int64_t nbase,
                                             int logd, float (*xch)[kWaves], float4 (&v)[V], float (&norm)[V]) {
  load_f4<V, FULL, true>(a.x, b, end, v);  // read once: non-temporal
  scale_f4<V>(v, a);
  bucket_norms<FULL, V>(a, b, end, tbegin, nbase, logd, xch, v, norm);
}

// Quantise V rows of the block at b against each row's own norm: quant_store (omf_qsgd_enc.h) with a norm per
// row (the draws and the level math are its: philox_rows, load_quad, qsgd_quad).  sink(k, e, qq): the four
// levels of the live quad (e < end) of row k at element e — the wire's store.
template <bool HAS_U, bool FULL, int V, class Sink>
__device__ __forceinline__ void quant_rows(const float4 (&v)[V], const EncArgs& a, int64_t b, int64_t end,
                                           int64_t tbegin, int32_t tensor, const float (&norm)[V], Sink sink) {
  static_assert(V % 4 == 0, "rows come in groups of 4 (RNG slots)");
#pragma unroll
  for (int g = 0; g < V / 4; ++g) {
    float4 uu[4];
    if (HAS_U) {
#pragma unroll
      for (int sl = 0; sl < 4; ++sl)
        uu[sl] = load_quad<FULL>(a.u, b + 4 * ((int64_t)(4 * g + sl) * kThreads + threadIdx.x), end);
    } else {
      philox_rows(a, b, tbegin, tensor, g, uu);
    }
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      const int k = 4 * g + sl;
      const int64_t e = b + 4 * ((int64_t)k * kThreads + threadIdx.x);
      if (!FULL && e >= end) continue;
      const Divisor dv(norm[k], kFmtF32);
      int32_t qq[4];
      qsgd_quad(v[k], uu[sl], dv, a.levels, !(norm[k] != 0.0f), qq);
      sink(k, e, qq);
    }
  }
}

// ---------------------------------------------------------------- the packed wire's back half
constexpr int kPackRows = 4;                           // rows of 1024 elements per workgroup
constexpr int kPackBlkElems = kPackRows * 4 * kThreads;  // 4096
constexpr int kPackBlkGroups = kPackBlkElems / 32;     // 128

// The back half of one block [b0, end) of tensor `tensor` on the bit-packed wire: the rows' levels (quant_rows)
// as codes into the LDS tile, one barrier, the block's words out.
// tile: kPackBlkElems / 4 8-byte fragment slots (slot k 256 + tid: the quad of row k, lane tid; group g's are
// slots 8 g .. 8 g + 7), or WIDE kPackBlkElems dwords (one per code, in element order).
template <bool HAS_U, bool FULL, bool WIDE>
__device__ __forceinline__ void pack_rows(const float4 (&v)[kPackRows], const float (&norm)[kPackRows], const EncArgs& a,
                                          int64_t b0, int64_t end, int64_t tbegin, int32_t tensor, uint32_t* tile,
                                          int bits, int32_t L, int mode) {
  const int tid = (int)threadIdx.x;
  uint64_t* frag = reinterpret_cast<uint64_t*>(tile);
  if (!FULL) {  // quads past the end hold code 0 (quant_rows skips them)
#pragma unroll
    for (int k = 0; k < kPackRows; ++k) {
      if (b0 + 4 * ((int64_t)k * kThreads + tid) < end) continue;
      if (WIDE) *reinterpret_cast<uint4*>(tile + 4 * (k * kThreads + tid)) = make_uint4(0u, 0u, 0u, 0u);
      else frag[k * kThreads + tid] = 0ull;
    }
  }
  quant_rows<HAS_U, FULL, kPackRows>(v, a, b0, end, tbegin, tensor, norm, [&](int k, int64_t e, const int32_t (&qq)[4]) {
    uint32_t code[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) code[c] = (FULL || e + c < end) ? qsgd_code(qq[c], L) : 0u;  // code 0 past the end
    if (WIDE) {
      *reinterpret_cast<uint4*>(tile + 4 * (k * kThreads + tid)) = make_uint4(code[0], code[1], code[2], code[3]);
    } else {  // the quad's fragment: 4 b <= 64 bits
      frag[k * kThreads + tid] = (uint64_t)code[0] | ((uint64_t)code[1] << bits) | ((uint64_t)code[2] << (2 * bits)) |
                                 ((uint64_t)code[3] << (3 * bits));
    }
  });
  __syncthreads();
  const int groups = FULL ? kPackBlkGroups : (int)((end - b0 + 31) >> 5);
  uint32_t* out = reinterpret_cast<uint32_t*>(a.q) + (b0 >> 5) * (int64_t)bits;  // b0 is a multiple of 32
  if (WIDE || mode == 0) {
    // thread i writes words i, i + 256, ...: word W is word W - g b of group g = floor(W / b)
    const int ub = WIDE ? bits : 4 * bits, n = WIDE ? 32 : 8, span = ub < 16 ? 4 : 3;
    const float inv_b = 1.0f / (float)bits, inv_ub = 1.0f / (float)ub;
    const int words = groups * bits;
    for (int W = tid; W < words; W += kThreads) {
      const int g = (int)(((float)W + 0.5f) * inv_b);  // exact: W < 4096, b <= 32 (group_word's argument)
      const uint32_t word = group_word(W - g * bits, ub, inv_ub, n, span, [&](int j) {
        return WIDE ? (uint64_t)tile[32 * g + j] : frag[8 * g + j];
      });
      store_nt(out + W, word);
    }
    return;
  }
  // two threads per group, each its half of the group's b words: the fragments walked in halves of 2 b <= 32
  // bits through a 64-bit accumulator, as qsgd_pack walks its levels
  const int g = tid >> 1;
  if (g >= groups) return;
  const int half = (bits + 1) >> 1;
  const int w0 = (tid & 1) ? half : 0, w1 = (tid & 1) ? bits : half;
  const int hb = 2 * bits;
  const uint64_t hm = (1ull << hb) - 1ull;
  uint64_t acc = 0;
  int nb = 0, w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint64_t f = frag[8 * g + j];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      acc |= (h ? f >> hb : f & hm) << nb;
      nb += hb;
      if (nb >= 32) {
        if (w >= w0 && w < w1) store_nt(out + g * bits + w, (uint32_t)acc);
        ++w;
        acc >>= 32;
        nb -= 32;
      }
    }
  }
}

// A payload quad (WIDTH 1: its dword of int8 levels in raw[0]; 4: raw[0..3]) decoded against its bucket's norm
// (omf_qsgd_bucketed.hip's sums, omf_qsgd_bucket_rot.hip's).
template <int WIDTH, bool POW2>
__device__ __forceinline__ void dec_quad(const int32_t* raw, float norm, float levels, float inv_levels, float (&yv)[4]) {
  int32_t qi[4];
  if (WIDTH == 1) {
    qsgd_split_i8(raw[0], qi);
  } else {
    qi[0] = raw[0]; qi[1] = raw[1]; qi[2] = raw[2]; qi[3] = raw[3];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) yv[c] = qsgd_dec_elem<POW2>(norm, qi[c], levels, inv_levels);
}

constexpr int kBucketSumMax = 8;  // clients per launch; the calls chain groups (sum_group, omf_qsgd_dec.h)
template <int N>
struct BSumArgs {  // SumArgs of omf_qsgd_recv.hip; q[k] is client k's payload (levels, or the packed words),
  const void* q[N];  // norm[k] its bucket-norm arena
  const float* norm[N];
  float* y;
  float levels, inv_levels;
  float divisor, pad_div;
  int32_t init, fill;
};

// What the receive calls of the int8 / int32 bucketed wire check before anything is launched (`who`: the entry
// point, `plain`: its one-client form); *logd: log2 of the bucket size.
inline int bucket_sum_checks(const omf_plan* p, const void* const* q, const float* const* bnorm, int32_t nclients,
                             int32_t width, int32_t levels, int64_t d, const float* y, bool plain, const std::string& who,
                             int* logd_out) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd = bucket::log2_size(d);
  if (logd < 0) return fail(OMF_EINVAL, kBucketBadSize);
  if (width != 8 && width != 32) return fail(OMF_EINVAL, "width must be 8 or 32");
  if (levels <= 0) return fail(OMF_EINVAL, "levels must be > 0");
  if (nclients < 1) return fail(OMF_EINVAL, who + ": nclients must be >= 1");
  if (!q || !bnorm || !y) return fail(OMF_EINVAL, "q, bnorm and y_out must be non-NULL");
  if (!aligned(y, 16)) return fail(OMF_EINVAL, kBucketMisaligned);
  const int64_t nb = bucket::offsets(p->sizes.data(), p->nt, logd, nullptr);
  const size_t ybytes = (size_t)p->arena_end * 4;
  const size_t qbytes = width == 8 ? (size_t)((p->arena_end + 3) & ~(int64_t)3) : (size_t)p->arena_end * 4;
  for (int32_t k = 0; k < nclients; ++k) {
    if (!q[k] || !bnorm[k]) return fail(OMF_EINVAL, who + (plain ? ": q and bnorm must be non-NULL" : ": a NULL entry in q or bnorm"));
    if (!aligned(q[k], width == 8 ? 4 : 16) || !aligned(bnorm[k], 4)) return fail(OMF_EINVAL, kBucketMisaligned);
    if (overlaps(y, ybytes, q[k], qbytes) || overlaps(y, ybytes, bnorm[k], (size_t)nb * 4))
      return fail(OMF_EINVAL, who + ": y_out overlaps a payload or norm buffer");
  }
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  *logd_out = logd;
  return OMF_OK;
}

// The plan's tables of bucket size 2^logd: boff on the device, nb on the host.  Built and uploaded at the
// first call at that size (synchronous), kept for the plan's life (at most bucket::kSizes of them): no later
// call allocates or synchronises.
inline int bucket_tables(omf_plan* p, int logd, const int64_t** boff, int64_t* nb) {
  const int i = logd - bucket::kMinLog2;
  if (!p->d_boff[i]) {
    std::vector<int64_t> h((size_t)p->nt);
    const int64_t total = bucket::offsets(p->sizes.data(), p->nt, logd, h.data());
    void* d = nullptr;
    OMF_HIP(hipMalloc(&d, h.size() * sizeof(int64_t)));
    if (const hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice); e != hipSuccess) {
      (void)hipFree(d);
      return hip_fail(e, "hipMemcpy(boff)");
    }
    p->d_lazy.push_back(d);  // the plan owns it
    p->d_boff[i] = static_cast<int64_t*>(d);
    p->bucket_nb[i] = total;
  }
  *boff = p->d_boff[i];
  *nb = p->bucket_nb[i];
  return OMF_OK;
}

}  // namespace
#endif  // __HIPCC__
