// omf_qsgd_bucket_h16.hip — bucketed QSGD encode of bf16 / fp16 tensors from a 16-bit arena, MI355X (gfx950): the
// product of omf_qsgd_bucketed.hip / omf_qsgd_bucket_pack.hip (bucket norms, one read of x) and omf_qsgd_h16.hip
// (the arena holds the tensors' own 16-bit patterns at the plan's element offsets, widened in registers).
// DESIGN.md §3.4f.
//
// Semantics: the values are widened exactly and everything after that is fp32 — v = fl32(alpha float(x16)),
// norm_b by the summation order of omf_qsgd_bucket.h, levels from qsgd_quad with Divisor(norm_b, kFmtF32) —
// so the norm bits and the payload bytes are omf_qsgd_encode_bucketed[_packed]'s on the exact fp32 upcast of
// the arena.  Nothing is rounded to the value format: EncArgs::fmt stays kFmtF32 (scale_f4 and Divisor round
// when it is not), and which 16-bit pattern x16 holds travels as a kernel argument of its own.
//
// Kernel map:
//   qsgd_bucket_encode_h16<WIDTH, HAS_U, V, LOGD>   qsgd_bucket_encode's workgroup, block and thread ->
//                    quad mapping (row k of the block at b is the quad at b + 4 (k 256 + tid); blocks start a
//                    multiple of 4096 elements after their tensor's begin), so bucket_norms, quant_rows and
//                    store_quad are that kernel's, untouched.  New is the front's data movement: a lane's quad is
//                    8 bytes, loaded non-temporally (x is read once) by load_h4 and widened in registers — bf16
//                    two shifts / masks per dword, fp16 one v_cvt_f32_f16 per half — behind ONE wave-uniform
//                    branch on the format around the loads, so the format does not double the instances.  A
//                    tensor's last quad (1-3 elements) and last dword (one element) are read element by element
//                    (load_hwords); nothing at or past a tensor's end is read.  A NULL q stops after the norms.
//                    Launch shapes: V = 4 rows per workgroup (the default: 32 B per thread in flight), or V = 8
//                    (64 B, the fp32 kernel's) when omf_plan_set_bucket_rows asks for 8: measured within each
//                    other's spread on Llama-400M (bf16, d = 512: 0.379 against 0.371 ms) and 4 rows 10 % faster
//                    on ResNet-18; 16-byte loads with a DPP pair swap were measured too (0.379 ms) and deleted
//                    (profiles/bucketed_h16_ab.json).  d is a compile-time parameter (LOGD =
//                    6 .. 12) in every instance.
//   qsgd_bucket_pack_h16<HAS_U, LOGD, PWIDE>   the same front (4 rows), then pack_rows (omf_qsgd_bucket.h): the back
//                    half of qsgd_bucket_encode_packed — codes into the LDS tile, one barrier, the block's words
//                    out.  PWIDE (b > 16): one LDS dword per code, d a kernel argument (LOGD = 0).
// No workgroup waits for another: no polling, no ticket, no atomic, no timeout.  No MFMA (no contraction).
// Traffic: 2 B read, 1 + 4 / d B (int8 wire) or b / 8 + 4 / d B (packed wire) written per element.
#include "../../include/omf_codec.h"
#include "omf_bracket.h"  // EncCall, enc_args, launch_kernel
#include "omf_common.h"
#include "omf_plan.h"
#include "omf_qsgd_bucket.h"
#include "omf_qsgd_enc.h"

using namespace omf;
using namespace omf::plan_layout;

namespace {

// The front half of one block [b, end) of V rows from the 16-bit arena x: bucket_front (omf_qsgd_bucket.h) with
// the rows loaded as 16-bit patterns and widened.  a.fmt is kFmtF32: the product with alpha is not rounded.
template <bool FULL, int V>
__device__ __forceinline__ void front_h16(const EncArgs& a, const uint16_t* __restrict__ x, bool bf16, int64_t b,
                                          int64_t end, int64_t tbegin, int64_t nbase, int logd, float (*xch)[kWaves],
                                          float4 (&v)[V], float (&norm)[V]) {
  if (bf16) load_h4<V, FULL, true, false, true>(x, b, end, v);  // wave-uniform
  else load_h4<V, FULL, true, false, false>(x, b, end, v);
  scale_f4<V>(v, a);
  bucket_norms<FULL, V>(a, b, end, tbegin, nbase, logd, xch, v, norm);
}

// ---------------------------------------------------------------- the int8 / int32 wire

template <int WIDTH, bool HAS_U, bool FULL, int V>
__device__ __forceinline__ void encode_block(const EncArgs& a, const uint16_t* __restrict__ x, bool bf16, int64_t b,
                                             int64_t end, int64_t tbegin, int32_t tensor, int64_t nbase, int logd,
                                             float (*xch)[kWaves]) {
  float4 v[V];
  float norm[V];
  front_h16<FULL, V>(a, x, bf16, b, end, tbegin, nbase, logd, xch, v, norm);
  if (!a.q) return;  // norms only (uniform)
  quant_rows<HAS_U, FULL, V>(v, a, b, end, tbegin, tensor, norm,
                             [&](int, int64_t e, const int32_t (&qq)[4]) { store_quad<WIDTH, FULL>(a, e, end, qq); });
}

template <int WIDTH, bool HAS_U, int V, int LOGD>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_encode_h16(EncArgs a, const uint16_t* __restrict__ x16, int bf16,
                                                                   const int64_t* __restrict__ boff) {
  constexpr int PER = (int)(kSub / ((int64_t)V * 1024));  // blocks per flat item
  __shared__ float xch[V][kWaves];
  const Item it = a.items[blockIdx.x / PER];
  const int64_t b = it.begin + (int64_t)(blockIdx.x % PER) * V * 1024;
  if (b >= it.end) return;
  const int64_t end = min(b + (int64_t)V * 1024, it.end);
  const int64_t tbegin = a.tinfo[it.tensor].begin;
  const int64_t nbase = boff[it.tensor];
  if (end - b == (int64_t)V * 1024)
    encode_block<WIDTH, HAS_U, true, V>(a, x16, bf16 != 0, b, end, tbegin, it.tensor, nbase, LOGD, xch);
  else
    encode_block<WIDTH, HAS_U, false, V>(a, x16, bf16 != 0, b, end, tbegin, it.tensor, nbase, LOGD, xch);
}

using EncodeKernel = void (*)(EncArgs, const uint16_t*, int, const int64_t*);

template <int V, int LOGD>
EncodeKernel encode_kernel_at(bool int32_wire, bool has_u) {
  static const EncodeKernel kern[2][2] = {
      {qsgd_bucket_encode_h16<1, false, V, LOGD>, qsgd_bucket_encode_h16<1, true, V, LOGD>},
      {qsgd_bucket_encode_h16<4, false, V, LOGD>, qsgd_bucket_encode_h16<4, true, V, LOGD>}};
  return kern[int32_wire][has_u];
}

template <int V>
EncodeKernel encode_kernel(int logd, bool w, bool u) {
  switch (logd) {
    case 6: return encode_kernel_at<V, 6>(w, u);
    case 7: return encode_kernel_at<V, 7>(w, u);
    case 8: return encode_kernel_at<V, 8>(w, u);
    case 9: return encode_kernel_at<V, 9>(w, u);
    case 10: return encode_kernel_at<V, 10>(w, u);
    case 11: return encode_kernel_at<V, 11>(w, u);
    default: return encode_kernel_at<V, 12>(w, u);
  }
}

// ---------------------------------------------------------------- the bit-packed wire

template <bool HAS_U, bool FULL, bool PWIDE>
__device__ __forceinline__ void pack_block(const EncArgs& a, const uint16_t* __restrict__ x, bool bf16, int64_t b0,
                                           int64_t end, int64_t tbegin, int32_t tensor, int64_t nbase, int logd,
                                           float (*xch)[kWaves], uint32_t* tile, int bits, int32_t L, int mode) {
  float4 v[kPackRows];
  float norm[kPackRows];
  front_h16<FULL, kPackRows>(a, x, bf16, b0, end, tbegin, nbase, logd, xch, v, norm);
  pack_rows<HAS_U, FULL, PWIDE>(v, norm, a, b0, end, tbegin, tensor, tile, bits, L, mode);
}

// LOGD: log2 d at compile time, or 0: the kernel argument (the PWIDE instances).
template <bool HAS_U, int LOGD, bool PWIDE>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_pack_h16(EncArgs a, const uint16_t* __restrict__ x16, int bf16,
                                                                 const int64_t* __restrict__ boff, int logd_arg, int bits,
                                                                 int32_t L, int mode) {
  const int logd = LOGD ? LOGD : logd_arg;
  constexpr int PER = (int)(kSub / kPackBlkElems);  // blocks per flat item
  __shared__ float xch[kPackRows][kWaves];
  __shared__ __attribute__((aligned(16))) uint32_t tile[PWIDE ? kPackBlkElems : kPackBlkElems / 2];
  const Item it = a.items[blockIdx.x / PER];
  const int64_t b0 = it.begin + (int64_t)(blockIdx.x % PER) * kPackBlkElems;
  if (b0 >= it.end) return;
  const int64_t end = min(b0 + (int64_t)kPackBlkElems, it.end);
  const int64_t tbegin = a.tinfo[it.tensor].begin;
  const int64_t nbase = boff[it.tensor];
  if (end - b0 == kPackBlkElems)
    pack_block<HAS_U, true, PWIDE>(a, x16, bf16 != 0, b0, end, tbegin, it.tensor, nbase, logd, xch, tile, bits, L, mode);
  else
    pack_block<HAS_U, false, PWIDE>(a, x16, bf16 != 0, b0, end, tbegin, it.tensor, nbase, logd, xch, tile, bits, L, mode);
}

using PackKernel = void (*)(EncArgs, const uint16_t*, int, const int64_t*, int, int, int32_t, int);

template <int LOGD, bool PWIDE = false>
PackKernel pack_kernel_at(bool has_u) {
  return has_u ? qsgd_bucket_pack_h16<true, LOGD, PWIDE> : qsgd_bucket_pack_h16<false, LOGD, PWIDE>;
}

PackKernel pack_kernel(int logd, bool pwide, bool u) {
  if (pwide) return pack_kernel_at<0, true>(u);
  switch (logd) {
    case 6: return pack_kernel_at<6>(u);
    case 7: return pack_kernel_at<7>(u);
    case 8: return pack_kernel_at<8>(u);
    case 9: return pack_kernel_at<9>(u);
    case 10: return pack_kernel_at<10>(u);
    case 11: return pack_kernel_at<11>(u);
    default: return pack_kernel_at<12>(u);
  }
}

// ---------------------------------------------------------------- host side

enum Wire { kLevels, kNormsOnly, kPacked };

// The checks of encode_bucketed (omf_qsgd_bucketed.hip) or encode_packed (omf_qsgd_bucket_pack.hip) with x16 and
// its format in place of x, then the one launch.
int encode_h16(omf_plan* p, const void* x16, int32_t fmt, float alpha, int32_t s, int64_t d, const float* u,
               uint64_t seed, uint64_t offset, const float* bnorm_in, void* q, float* bnorm_out, Wire wire, void* stream) {
  if (fmt != 1 && fmt != 2) return fail(OMF_EINVAL, "value_format of a 16-bit arena must be 1 (bf16) or 2 (fp16)");
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd = bucket::log2_size(d);
  if (logd < 0) return fail(OMF_EINVAL, kBucketBadSize);
  if (s < 0 || s > 30) return fail(OMF_EINVAL, "bit_width must be in [0, 30] (levels = 2^bit_width is an int32 on the wire)");
  const int width = wire == kPacked ? 0 : ((1 << s) <= 127 ? 1 : 4);
  if (wire == kPacked) {
    if (!x16 || !bnorm_out || !q) return fail(OMF_EINVAL, "x16, packed_out and bnorm_out must be non-NULL");
    if (!aligned(x16, 16) || (u && !aligned(u, 16)) || !aligned(q, 8))
      return fail(OMF_EINVAL, "x16 and u must be 16-byte, packed_out 8-byte aligned");
  } else {
    if (!x16 || !bnorm_out || (wire != kNormsOnly && !q)) return fail(OMF_EINVAL, "x16, q and bnorm_out must be non-NULL");
    if (!aligned(x16, 16) || (u && !aligned(u, 16)) || (q && !aligned(q, width == 1 ? 4 : 16)))
      return fail(OMF_EINVAL, kBucketMisaligned);
  }
  if (!aligned(bnorm_out, 4) || (bnorm_in && !aligned(bnorm_in, 4))) return fail(OMF_EINVAL, "misaligned bucket norms");
  if (wire == kPacked) {
    ArenaArgs arena;
    dim3 unused;
    if (const int rc = packed_arena(p, &arena, &unused)) return rc;  // offsets that are multiples of 32
  }
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  const int64_t* boff = nullptr;
  int64_t nb = 0;
  if (int r = bucket_tables(p, logd, &boff, &nb)) return r;
  const hipStream_t st = (hipStream_t)stream;
  // fmt of the call record stays kFmtF32: no rounding to the value format anywhere
  EncArgs a = enc_args(p, EncCall{nullptr, alpha, s, u, seed, offset, bnorm_in, wire == kNormsOnly ? nullptr : q, bnorm_out,
                                  wire == kNormsOnly, st, 0.0f, nullptr, kFmtF32, nullptr, width});
  a.items = p->d_flat;
  a.tinfo = p->d_tinfo[0];
  const uint16_t* x = static_cast<const uint16_t*>(x16);
  const int bf16 = fmt == 1;
  const bool hu = u != nullptr;
  if (wire == kPacked) {
    const unsigned blocks = (unsigned)(p->n_flat * (kSub / kPackBlkElems));
    const int32_t L = (int32_t)1 << s;
    const int bits = omf_qsgd_packed_bits(L);  // s + 2
    launch_kernel(pack_kernel(logd, bits > 16, hu), dim3(blocks), dim3(kThreads), 0, st, a, x, bf16, boff, logd, bits, L, (int)p->bucket_pack);
  } else {
    const bool w = width == 4;
    const int rows = p->bucket_rows == 8 ? 8 : 4;
    const unsigned blocks = (unsigned)(p->n_flat * (kSub / (rows * 1024)));
    const EncodeKernel k = rows == 8 ? encode_kernel<8>(logd, w, hu) : encode_kernel<4>(logd, w, hu);
    launch_kernel(k, dim3(blocks), dim3(kThreads), 0, st, a, x, bf16, boff);
  }
  OMF_HIP(hipGetLastError());
  if (wire != kNormsOnly) p->last_encoder = wire == kPacked ? kEncBucketedPackedH16 : kEncBucketedH16;
  return OMF_OK;
}

}  // namespace

extern "C" {

int omf_qsgd_encode_bucketed_h16(omf_plan* plan, const void* x16, int32_t value_format, float alpha, int32_t bit_width,
                                 int64_t bucket_size, const float* u, uint64_t seed, uint64_t offset,
                                 const float* bnorm_in, void* q_out, float* bnorm_out, void* stream) {
  return encode_h16(plan, x16, value_format, alpha, bit_width, bucket_size, u, seed, offset, bnorm_in, q_out, bnorm_out,
                    kLevels, stream);
}

int omf_qsgd_norms_bucketed_h16(omf_plan* plan, const void* x16, int32_t value_format, float alpha, int64_t bucket_size,
                                float* bnorm_out, void* stream) {
  return encode_h16(plan, x16, value_format, alpha, 0, bucket_size, nullptr, 0, 0, nullptr, nullptr, bnorm_out, kNormsOnly,
                    stream);
}

int omf_qsgd_encode_bucketed_packed_h16(omf_plan* plan, const void* x16, int32_t value_format, float alpha,
                                        int32_t bit_width, int64_t bucket_size, const float* u, uint64_t seed,
                                        uint64_t offset, const float* bnorm_in, uint32_t* packed_out, float* bnorm_out,
                                        void* stream) {
  return encode_h16(plan, x16, value_format, alpha, bit_width, bucket_size, u, seed, offset, bnorm_in, packed_out,
                    bnorm_out, kPacked, stream);
}

}  // extern "C"
