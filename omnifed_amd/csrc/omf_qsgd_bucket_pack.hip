// omf_qsgd_bucket_pack.hip — bucketed QSGD on the bit-packed wire ("QSGDBucketedPackedCompression"), MI355X
// (gfx950): the bucketed encoder that packs its codes inside the encode pass, and the packed bucketed decoder /
// K-client decode-and-sum, with their host side.  The wire is the product of two existing ones: bucket norms
// as omf_qsgd_bucketed.hip writes them (omf_qsgd_bucket.h: d, boff, the summation order), codes as
// omf_qsgd_pack.hip packs them (code q + L in b = packed_bits(L) bits, LSB first, 32 elements = b words,
// tensor t at word offsets[t] b / 32, code 0 after a tensor's last element inside its last group, groups
// without a tensor element not written).  DESIGN.md §3.4d.
//
// Kernel map:
//   qsgd_bucket_encode_packed<HAS_U, LOGD, WIDE>   qsgd_bucket_encode's workgroup (256 threads, 4 rows of 1024
//                    elements) and front half (bucket_front, omf_qsgd_bucket.h: x read once, the bucket's norm
//                    in every lane of the bucket, stored by its first lane) and its quantiser (quant_rows).  A
//                    workgroup owns whole buckets and waits for nobody, so a lane's levels are final in
//                    registers: instead of storing them, each lane folds its quad's four codes into one
//                    fragment of 4 b bits (b <= 16: an 8-byte LDS slot per quad, 4 x 256 slots = 8 KiB), one
//                    workgroup barrier follows (the only one besides bucket_sums' from d = 512 up), and
//                    threads assemble whole output words from the slots (group_word, omf_qsgd_dec.h: a
//                    32-element group is 8 consecutive lanes of one row, its b words the concatenation of
//                    their fragments).  A full block leaves as 128 b contiguous words of the packed arena.
//                    Two output assignments (omf_plan_set_bucket_pack): 0 thread i writes words i, i + 256,
//                    ... of the block (lane-contiguous non-temporal 4-byte stores; the word's group is a
//                    multiplication by 1 / b); 1 two threads per group, each walking the group's fragments
//                    as qsgd_pack walks its levels and storing its half of the b words (no division).
//                    WIDE (b > 16, bit_width 8 .. 30): one LDS dword per code (16 KiB), words assembled
//                    from codes, assignment 0 only, d a kernel argument.
//                    No workgroup waits for another: no polling, no ticket, no atomic, no timeout.
//   qsgd_bucket_decode_sum_packed<B, POW2, N>   packed_sum_block (omf_qsgd_dec.h: qsgd_decode_sum_packed's
//                    body) with a thread's norm for client c gathered from
//                    bnorm_c[boff[t] + ((e0 - begins[t]) >> log2 d)]: a 32-element group lies in one tensor
//                    and one bucket (offsets are multiples of 32, d >= 64).  The plain decode is its N = 1
//                    launch that starts from y (accumulate) or from +0, without the padding fill.
//   qsgd_bucket_sum_packed_tiny   the same for an arena of fewer than 32 elements, element by element.
//
// HBM-bound; no MFMA (no contraction).  Encode traffic: 4 B read, b / 8 + 4 / d B written per element.
#include <algorithm>
#include <string>

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

constexpr int kRows = kPackRows;          // rows of 1024 elements per workgroup
constexpr int kBlkElems = kPackBlkElems;  // 4096

// One block [b0, end) of tensor `tensor`: norms (bucket_front), then levels, codes into the LDS tile and the
// block's words out (pack_rows, omf_qsgd_bucket.h).
template <bool HAS_U, bool FULL, bool WIDE>
__device__ __forceinline__ void pack_block(const EncArgs& a, int64_t b0, int64_t end, int64_t tbegin, int32_t tensor,
                                           int64_t nbase, int logd, float (*xch)[kWaves], uint32_t* tile, int bits,
                                           int32_t L, int mode) {
  float4 v[kRows];
  float norm[kRows];
  bucket_front<FULL, kRows>(a, b0, end, tbegin, nbase, logd, xch, v, norm);
  pack_rows<HAS_U, FULL, WIDE>(v, norm, a, b0, end, tbegin, tensor, tile, bits, L, mode);
}

// LOGD: log2 d at compile time, or 0: the kernel argument (the WIDE instances).
template <bool HAS_U, int LOGD, bool WIDE>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_encode_packed(EncArgs a, const int64_t* __restrict__ boff,
                                                                      int logd_arg, int bits, int32_t L, int mode) {
  const int logd = LOGD ? LOGD : logd_arg;
  constexpr int PER = (int)(kSub / kBlkElems);  // blocks per flat item
  __shared__ float xch[kRows][kWaves];
  __shared__ __attribute__((aligned(16))) uint32_t tile[WIDE ? kBlkElems : kBlkElems / 2];
  const Item it = a.items[blockIdx.x / PER];
  const int64_t b0 = it.begin + (int64_t)(blockIdx.x % PER) * kBlkElems;
  if (b0 >= it.end) return;
  const int64_t end = min(b0 + (int64_t)kBlkElems, it.end);
  const int64_t tbegin = a.tinfo[it.tensor].begin;
  const int64_t nbase = boff[it.tensor];
  if (end - b0 == kBlkElems) pack_block<HAS_U, true, WIDE>(a, b0, end, tbegin, it.tensor, nbase, logd, xch, tile, bits, L, mode);
  else pack_block<HAS_U, false, WIDE>(a, b0, end, tbegin, it.tensor, nbase, logd, xch, tile, bits, L, mode);
}

using PackKernel = void (*)(EncArgs, const int64_t*, int, int, int32_t, int);

template <int LOGD>
PackKernel narrow_kernel(bool has_u) {
  return has_u ? qsgd_bucket_encode_packed<true, LOGD, false> : qsgd_bucket_encode_packed<false, LOGD, false>;
}

PackKernel encode_kernel(int logd, bool wide, bool u) {
  if (wide) return u ? qsgd_bucket_encode_packed<true, 0, true> : qsgd_bucket_encode_packed<false, 0, true>;
  switch (logd) {
    case 6: return narrow_kernel<6>(u);
    case 7: return narrow_kernel<7>(u);
    case 8: return narrow_kernel<8>(u);
    case 9: return narrow_kernel<9>(u);
    case 10: return narrow_kernel<10>(u);
    case 11: return narrow_kernel<11>(u);
    default: return narrow_kernel<12>(u);
  }
}

// ---------------------------------------------------------------- decode and sum

constexpr int kSumMaxWide = 4;  // clients per launch of the runtime-width instance (b > 10), as omf_qsgd_pack.hip's

template <int B, bool POW2, int N>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_decode_sum_packed(
    BSumArgs<N> a, int32_t L, int32_t b_rt, const uint32_t* __restrict__ binfo, int64_t nbinfo,
    const int64_t* __restrict__ begins, const int64_t* __restrict__ sizes, const int64_t* __restrict__ boff, int logd,
    int32_t nt, int64_t arena_end) {
  __shared__ float tile[kThreads * 33];
  __shared__ int32_t s_lim[kThreads];
  packed_sum_block<B, POW2, N>(
      a, L, b_rt, [&](int c) { return static_cast<const uint32_t*>(a.q[c]); },
      [&](int c, int lim, int32_t t, int64_t e0) {  // the group's bucket: one gather per client
        return lim > 0 ? a.norm[c][boff[t] + ((e0 - begins[t]) >> logd)] : 0.0f;
      },
      binfo, nbinfo, begins, sizes, nt, arena_end, tile, s_lim);
}

// An arena of fewer than 32 elements (one group, one bucket per tensor): one thread per element, its code from
// at most two words of the group's b, `n` clients behind a uniform guard.
template <bool POW2>
__global__ __launch_bounds__(64) void qsgd_bucket_sum_packed_tiny(BSumArgs<kBucketSumMax> a, int32_t n, int32_t L,
                                                                  int32_t b, const int64_t* __restrict__ begins,
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
  const int64_t ni = boff[t];  // i - begins[t] < 32 < d: the tensor's first bucket
  const int bit = (int)(i & 31) * b, wi = bit >> 5;
  const int64_t woff = (i >> 5) * (int64_t)b;
  const uint64_t mask = (1ull << b) - 1ull;
  float s = a.init ? a.y[i] : 0.0f;
#pragma unroll
  for (int c = 0; c < kBucketSumMax; ++c) {
    if (c < n) {
      const uint32_t* p = static_cast<const uint32_t*>(a.q[c]) + woff;
      const uint64_t two = ((uint64_t)p[min(wi + 1, b - 1)] << 32) | p[wi];
      const uint32_t code = (uint32_t)((two >> (bit & 31)) & mask);
      s = __fadd_rn(s, qsgd_dec_elem<POW2>(a.norm[c][ni], qsgd_level(code, L), a.levels, a.inv_levels));
    }
  }
  a.y[i] = a.divisor != 0.0f ? s / a.divisor : s;
}

// ---------------------------------------------------------------- host side

int encode_packed(omf_plan* p, const float* x, float alpha, int32_t s, int64_t d, const float* u, uint64_t seed,
                  uint64_t offset, const float* bnorm_in, uint32_t* packed, float* bnorm_out, void* stream) {
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd = bucket::log2_size(d);
  if (logd < 0) return fail(OMF_EINVAL, kBucketBadSize);
  if (s < 0 || s > 30) return fail(OMF_EINVAL, "bit_width must be in [0, 30] (levels = 2^bit_width is an int32 on the wire)");
  if (!x || !bnorm_out || !packed) return fail(OMF_EINVAL, "x, packed_out and bnorm_out must be non-NULL");
  if (!aligned(x, 16) || (u && !aligned(u, 16)) || !aligned(packed, 8))
    return fail(OMF_EINVAL, "x and u must be 16-byte, packed_out 8-byte aligned");
  if (!aligned(bnorm_out, 4) || (bnorm_in && !aligned(bnorm_in, 4))) return fail(OMF_EINVAL, "misaligned bucket norms");
  ArenaArgs arena;
  dim3 unused;
  if (const int rc = packed_arena(p, &arena, &unused)) return rc;  // offsets that are multiples of 32
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const int64_t* boff = nullptr;
  int64_t nb = 0;
  if (int r = bucket_tables(p, logd, &boff, &nb)) return r;
  const hipStream_t st = (hipStream_t)stream;
  const int32_t L = (int32_t)1 << s;
  const int bits = omf_qsgd_packed_bits(L);  // s + 2
  EncArgs a = enc_args(p, EncCall{x, alpha, s, u, seed, offset, bnorm_in, packed, bnorm_out, false, st, 0.0f, nullptr, 0u,
                                  nullptr, 0});
  a.items = p->d_flat;
  a.tinfo = p->d_tinfo[0];
  const unsigned blocks = (unsigned)(p->n_flat * (kSub / kBlkElems));
  launch_kernel(encode_kernel(logd, bits > 16, u != nullptr), dim3(blocks), dim3(kThreads), 0, st, a, boff, logd, bits, L,
                (int)p->bucket_pack);
  OMF_HIP(hipGetLastError());
  p->last_encoder = kEncBucketedPacked;
  return OMF_OK;
}

struct PSumCall : SumCallBase {
  const omf_plan* p;
  ArenaArgs a;
  dim3 grid;
  const uint32_t* const* packed;
  const int64_t* boff;
  int logd;
  int32_t L, b;
};

template <int N>
BSumArgs<N> sum_args(const PSumCall& c, int n) {
  BSumArgs<N> a{};
  for (int k = 0; k < n; ++k) a.q[k] = c.packed[k];
  sum_common_args(a, c, n);
  return a;
}

template <bool P>
void launch_sum(const PSumCall& c) {
  const int n = c.g.n;
  if (c.a.arena_end < 32) {  // no whole group: the element kernel
    hipLaunchKernelGGL((qsgd_bucket_sum_packed_tiny<P>), dim3(1), dim3(64), 0, c.st, sum_args<kBucketSumMax>(c, n), n, c.L,
                       c.b, c.a.begins, c.a.sizes, c.boff, c.a.nt, c.a.arena_end);
    return;
  }
  with_code_bits(c.b, [&](auto B) {
    with_group_size<(B() != 0 ? kBucketSumMax : kSumMaxWide)>(n, [&](auto N) {
      hipLaunchKernelGGL((qsgd_bucket_decode_sum_packed<B(), P, N()>), c.grid, dim3(kThreads), 0, c.st,
                         sum_args<N()>(c, N()), c.L, c.b, c.a.binfo, c.a.nbinfo, c.a.begins, c.a.sizes, c.boff, c.logd,
                         c.a.nt, c.a.arena_end);
    });
  });
}

// The checks both receive calls share, then the chained groups.  `plain`: omf_qsgd_decode_bucketed_packed's one
// client, which never fills the padding.
int sum_packed(omf_plan* p, const uint32_t* const* packed, const float* const* bnorm, int32_t nclients, int32_t levels,
               int64_t d, float* y, int32_t init, float divisor, bool plain, void* stream) {
  const std::string who = plain ? "omf_qsgd_decode_bucketed_packed" : "omf_qsgd_decode_sum_bucketed_packed";
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd = bucket::log2_size(d);
  if (logd < 0) return fail(OMF_EINVAL, kBucketBadSize);
  const int32_t b = omf_qsgd_packed_bits(levels);
  if (b < 0 || b > 32) return fail(OMF_EINVAL, "levels must be in [1, 2^31 - 1)");
  if (nclients < 1) return fail(OMF_EINVAL, who + ": nclients must be >= 1");
  if (!packed || !bnorm || !y) return fail(OMF_EINVAL, "packed, bnorm and y_out must be non-NULL");
  if (!aligned(y, 16)) return fail(OMF_EINVAL, "y_out must be 16-byte aligned");
  PSumCall c;
  if (const int rc = packed_arena(p, &c.a, &c.grid)) return rc;
  const int64_t nb = bucket::offsets(p->sizes.data(), p->nt, logd, nullptr);
  const size_t ybytes = (size_t)p->arena_end * 4;
  const size_t pbytes = (size_t)((p->arena_end + 31) / 32) * (size_t)b * 4;
  for (int32_t k = 0; k < nclients; ++k) {
    if (!packed[k] || !bnorm[k]) return fail(OMF_EINVAL, who + (plain ? ": packed and bnorm must be non-NULL" : ": a NULL entry in packed or bnorm"));
    if (!aligned(packed[k], 4) || !aligned(bnorm[k], 4)) return fail(OMF_EINVAL, "a packed arena and its bucket norms must be 4-byte aligned");
    if (overlaps(y, ybytes, packed[k], pbytes) || overlaps(y, ybytes, bnorm[k], (size_t)nb * 4))
      return fail(OMF_EINVAL, who + ": y_out overlaps a packed or norm buffer");
  }
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const LevelScale lv(levels);
  int64_t nb_table = 0;
  if (int r = bucket_tables(p, logd, &c.boff, &nb_table)) return r;
  c.p = p; c.y = y; c.st = (hipStream_t)stream; c.levels = lv.levels; c.inv_levels = lv.inv_levels; c.logd = logd;
  c.L = levels; c.b = b;
  const int32_t per = b <= 10 ? kBucketSumMax : kSumMaxWide;
  for (int32_t k0 = 0; k0 < nclients; k0 += per) {  // the chained groups (sum_group, omf_qsgd_dec.h)
    c.g = sum_group(nclients, per, init, divisor, k0);
    if (plain) c.g.fill = 0;
    c.packed = packed + k0; c.norm = bnorm + k0;
    if (lv.pow2) launch_sum<true>(c); else launch_sum<false>(c);
    OMF_HIP(hipGetLastError());
  }
  return OMF_OK;
}

}  // namespace

extern "C" {

int omf_qsgd_encode_bucketed_packed(omf_plan* plan, const float* x, float alpha, int32_t bit_width, int64_t bucket_size,
                                    const float* u, uint64_t seed, uint64_t offset, const float* bnorm_in,
                                    uint32_t* packed_out, float* bnorm_out, void* stream) {
  return encode_packed(plan, x, alpha, bit_width, bucket_size, u, seed, offset, bnorm_in, packed_out, bnorm_out, stream);
}

int omf_qsgd_decode_bucketed_packed(omf_plan* plan, const uint32_t* packed, int32_t levels, int64_t bucket_size,
                                    const float* bnorm, float* y_out, int32_t accumulate, void* stream) {
  return sum_packed(plan, &packed, &bnorm, 1, levels, bucket_size, y_out, accumulate, 0.0f, true, stream);
}

int omf_qsgd_decode_sum_bucketed_packed(omf_plan* plan, const uint32_t* const* packed, const float* const* bnorm,
                                        int32_t nclients, int32_t levels, int64_t bucket_size, float* y_out,
                                        int32_t init, float divisor, void* stream) {
  return sum_packed(plan, packed, bnorm, nclients, levels, bucket_size, y_out, init, divisor, false, stream);
}

int omf_plan_set_bucket_pack(omf_plan* plan, int32_t mode) {
  if (!plan) return fail(OMF_EINVAL, "plan is NULL");
  if (mode != 0 && mode != 1) return fail(OMF_EINVAL, "omf_plan_set_bucket_pack: mode must be 0 or 1");
  plan->bucket_pack = mode;
  return OMF_OK;
}

}  // extern "C"
