// omf_qsgd_bucket_ps.hip — the parameter server's step for bucketed QSGD, MI355X (gfx950): K clients' bucketed
// payloads (int8 / int32 levels or bit-packed codes) decoded, summed in client order onto the accumulator, divided
// and re-encoded with bucket norms — on the int8 / int32 or the bit-packed wire — in ONE launch in which the
// average never returns from HBM, with its host side (omf_ps_sum_encode_bucketed).  DESIGN.md §3.4e.
//
// Kernel map:
//   qsgd_bucket_ps<IN, OUT, N>   the bucketed encoder's work split (omf_qsgd_bucketed.hip): one 256-thread
//                    workgroup per block of 4 rows (4096 elements) of a flat 16 Ki item, row k of the block at b
//                    the quad at b + 4 (k 256 + tid), blocks a multiple of 4096 elements after their tensor's
//                    begin.  A block lies in one tensor, so the tensor, its begin and both bucket-arena offsets
//                    come from the block's Item: uniform loads, no table walk.
//                    Front half (ps_front), every global load issued before the first use: per row and client
//                    the quad's levels (IN = 1: one dword of int8; IN = 4: one 16-byte load) and its bucket's
//                    norm bnorm_c[boff_in[t] + ((e - tbegin) >> log2 d_in)], and the accumulator's quad when
//                    there is one.  IN = 0 (packed codes of b <= 16 bits): a block's codes of one client are
//                    128 b contiguous words; the workgroup fetches them lane-contiguous (thread i words i,
//                    i + 256, ...: each HBM word once, full-width) into an LDS tile per client, one barrier,
//                    then every lane extracts its quads' four codes from its group's words (group_quad,
//                    omf_qsgd_dec.h, the mirror image of group_word).  The sum runs in registers in client
//                    order from the accumulator (or +0), is stored to sum_out if asked, divided, masked to +0
//                    past the block's end and stored to avg_out (non-temporal).
//                    Back half, the encoders' code unchanged (omf_qsgd_bucket.h): bucket_norms (bucket_sums,
//                    the first lane's norm store), then quant_rows with store_quad (OUT = 1 / 4) or pack_rows
//                    (OUT = 0: fragments -> LDS -> group_word -> lane-contiguous non-temporal word stores).
//                    N, the clients of the launch, is a template parameter (exact-N instances, 0 .. 8): each
//                    client's pointers are compile-time fields of the kernel argument, and no padding client is
//                    needed (a +0 term would turn a -0 sum into +0).  d_in and d_out are kernel arguments.
//                    No workgroup waits for another: no polling, no ticket, no atomic, no timeout.
//   ps_map           dst = src (or +0), optionally / divisor, on the tensors' elements only: seeds and finishes
//                    the chained and fallback sequences, which must not write padding.
//
// HBM-bound; no MFMA (no contraction).  Traffic per element at K clients: K (w_in + 4 / d_in) read (+ 4 with an
// accumulator), 4 written (+ 4 with sum_out), w_out + 4 / d_out written; w = 1, 4 or b / 8 bytes.
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

constexpr int kRows = kPackRows;          // rows of 1024 elements per workgroup
constexpr int kBlkElems = kPackBlkElems;  // 4096
constexpr int kInTileWords = 8192;        // 32 KiB: N clients' 128 b words each, N b <= 64

// Clients per launch: registers bound the int8 / int32 wires (N quads of levels and N norms per row in flight),
// the LDS tile the packed wire.
constexpr int kPsMaxI8 = 8, kPsMaxI32 = 4, kPsMaxPacked = 8, kPsMaxPackedWide = 4;  // wide: b > 8

template <int N>
struct PsArgs {
  const void* q[N ? N : 1];       // client c's payload arena (levels, or packed words)
  const float* bnorm[N ? N : 1];  // its bucket-norm arena
  const float* acc;               // the sum's start, or NULL: +0
  float* sum_out;                 // NULL: the sum is not stored
  float* avg_out;
  const int64_t* boff_in;         // the tensors' offsets into a bucket-norm arena of size d_in
  float divisor;                  // 0: no division
  float levels, inv_levels;       // fl32(L_in), 2^-s_in
  int32_t L_in, bits_in, logd_in;
};

// A thread's words of one client's block on the packed wire: words tid, tid + 256, ... of the block's `words`.
// N > 4 means b <= 8: at most 1024 words a block.
template <int N>
constexpr int ps_words_per_thread() { return N > 4 ? 4 : 8; }

// The front half of one block [b0, end): the sum over the clients and its average, v (+0 past the end).
template <int IN, int N, bool FULL>
__device__ __forceinline__ void ps_front(const PsArgs<N>& s, int64_t b0, int64_t end, int64_t tbegin, int64_t nbase_in,
                                         uint32_t* in_tile, float4 (&v)[kRows]) {
  const int tid = (int)threadIdx.x;
  constexpr int NC = N ? N : 1;
  constexpr int RAW = IN == 4 ? 4 : 1;
  constexpr int WPT = ps_words_per_thread<N>();
  int32_t raw[NC][kRows][RAW];
  uint32_t wd[NC][IN == 0 ? WPT : 1];
  float norm[NC][kRows];
  float4 sum[kRows];
  const int b = s.bits_in;
  const int words = (FULL ? kPackBlkGroups : (int)((end - b0 + 31) >> 5)) * b;  // of one client's block (IN = 0)
  // ---- every global load
  if (N > 0 && IN == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const uint32_t* p = static_cast<const uint32_t*>(s.q[c]) + (b0 >> 5) * (int64_t)b;  // b0 is a multiple of 32
#pragma unroll
      for (int i = 0; i < WPT; ++i) {
        const int W = tid + i * kThreads;
        wd[c][i] = W < words ? __builtin_nontemporal_load(p + W) : 0u;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = b0 + 4 * ((int64_t)k * kThreads + tid);
    const bool live = FULL || e < end;
    if (N > 0) {
#pragma unroll
      for (int c = 0; c < N; ++c) {
        norm[c][k] = live ? s.bnorm[c][nbase_in + ((e - tbegin) >> s.logd_in)] : 0.0f;
        if (IN == 0) continue;
#pragma unroll
        for (int j = 0; j < RAW; ++j) raw[c][k][j] = 0;
        if (FULL || e + 4 <= end) {
          if (IN == 1) {
            raw[c][k][0] = *reinterpret_cast<const int32_t*>(static_cast<const int8_t*>(s.q[c]) + e);
          } else {
            const i32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(static_cast<const int32_t*>(s.q[c]) + e));
#pragma unroll
            for (int j = 0; j < RAW; ++j) raw[c][k][j] = t[j];
          }
        } else if (live) {  // the tensor's partial last quad: the payload may end with it
          int32_t rr[4] = {0, 0, 0, 0};
          qsgd_last_quad<(IN == 4 ? 4 : 1)>(s.q[c], e, end, rr);
#pragma unroll
          for (int j = 0; j < RAW; ++j) raw[c][k][j] = rr[j];
        }
      }
    }
    sum[k] = s.acc ? load_quad<FULL, true>(s.acc, e, end) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  // ---- the packed wire: the clients' words through the LDS tile
  if (N > 0 && IN == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
#pragma unroll
      for (int i = 0; i < WPT; ++i) {
        const int W = tid + i * kThreads;
        if (W < words) in_tile[c * kPackBlkGroups * b + W] = wd[c][i];
      }
    }
    __syncthreads();
  }
  // ---- sum in client order, divide
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = b0 + 4 * ((int64_t)k * kThreads + tid);
    const bool live = FULL || e < end;
    float sj[4] = {sum[k].x, sum[k].y, sum[k].z, sum[k].w};
    if (N > 0) {
#pragma unroll
      for (int c = 0; c < N; ++c) {
        int32_t qi[4] = {0, 0, 0, 0};
        if (IN == 0) {
          if (live) {  // group k 32 + tid / 8 of the block, quad tid % 8 of the group
            const uint32_t* gw = in_tile + (c * kPackBlkGroups + k * 32 + (tid >> 3)) * b;
            uint32_t code[4];
            group_quad(tid & 7, b, [&](int i) { return gw[i]; }, code);
#pragma unroll
            for (int j = 0; j < 4; ++j) qi[j] = qsgd_level(code[j], s.L_in);
          }
        } else if (IN == 1) {
          qsgd_split_i8(raw[c][k][0], qi);
        } else {
#pragma unroll
          for (int j = 0; j < RAW; ++j) qi[j] = raw[c][k][j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) sj[j] = __fadd_rn(sj[j], qsgd_dec_elem<true>(norm[c][k], qi[j], s.levels, s.inv_levels));
      }
    }
    float vj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vj[j] = s.divisor != 0.0f ? sj[j] / s.divisor : sj[j];
      if (!FULL && e + j >= end) vj[j] = 0.0f;  // whatever the codes say: a packed code 0 is level -L
    }
    v[k] = make_float4(vj[0], vj[1], vj[2], vj[3]);
    if (!live) continue;
    if (FULL || e + 4 <= end) {
      if (s.sum_out) *reinterpret_cast<float4*>(s.sum_out + e) = make_float4(sj[0], sj[1], sj[2], sj[3]);
      store_nt(s.avg_out + e, v[k]);
    } else {
      for (int j = 0; j < 3; ++j) {
        if (e + j >= end) break;
        if (s.sum_out) s.sum_out[e + j] = sj[j];
        s.avg_out[e + j] = vj[j];
      }
    }
  }
}

template <int IN, int OUT, int N, bool FULL>
__device__ __forceinline__ void ps_block(const EncArgs& a, const PsArgs<N>& s, int64_t b0, int64_t end, int64_t tbegin,
                                         int32_t tensor, int64_t nbase_in, int64_t nbase_out, int logd_out,
                                         float (*xch)[kWaves], uint32_t* in_tile, uint32_t* out_tile, int bits_out,
                                         int32_t L_out, int mode) {
  float4 v[kRows];
  float norm[kRows];
  ps_front<IN, N, FULL>(s, b0, end, tbegin, nbase_in, in_tile, v);
  bucket_norms<FULL, kRows>(a, b0, end, tbegin, nbase_out, logd_out, xch, v, norm);
  if (OUT == 0) {
    pack_rows<false, FULL, false>(v, norm, a, b0, end, tbegin, tensor, out_tile, bits_out, L_out, mode);
  } else {
    quant_rows<false, FULL, kRows>(v, a, b0, end, tbegin, tensor, norm,
                                   [&](int, int64_t e, const int32_t (&qq)[4]) { store_quad<OUT, FULL>(a, e, end, qq); });
  }
}

// IN / OUT: 1 int8, 4 int32, 0 packed (b <= 16).  a: the output side as the bucketed encoders take it (q, norm_out,
// levels, the Philox key; alpha = 1, no x, u or norm_in).
template <int IN, int OUT, int N>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_ps(EncArgs a, PsArgs<N> s, const int64_t* __restrict__ boff_out,
                                                           int logd_out, int bits_out, int32_t L_out, int mode) {
  constexpr int PER = (int)(kSub / kBlkElems);  // blocks per flat item
  __shared__ float xch[kRows][kWaves];
  __shared__ __attribute__((aligned(16))) uint32_t in_tile[(IN == 0 && N > 0) ? kInTileWords : 4];
  __shared__ __attribute__((aligned(16))) uint32_t out_tile[OUT == 0 ? kBlkElems / 2 : 4];
  const Item it = a.items[blockIdx.x / PER];
  const int64_t b0 = it.begin + (int64_t)(blockIdx.x % PER) * kBlkElems;
  if (b0 >= it.end) return;
  const int64_t end = min(b0 + (int64_t)kBlkElems, it.end);
  const int64_t tbegin = a.tinfo[it.tensor].begin;
  const int64_t nbase_out = boff_out[it.tensor];
  const int64_t nbase_in = N > 0 ? s.boff_in[it.tensor] : 0;
  if (end - b0 == kBlkElems)
    ps_block<IN, OUT, N, true>(a, s, b0, end, tbegin, it.tensor, nbase_in, nbase_out, logd_out, xch, in_tile, out_tile,
                               bits_out, L_out, mode);
  else
    ps_block<IN, OUT, N, false>(a, s, b0, end, tbegin, it.tensor, nbase_in, nbase_out, logd_out, xch, in_tile, out_tile,
                                bits_out, L_out, mode);
}

// dst = src (NULL: +0), / divisor unless 0, on the tensors' elements of the block; dst may be src.
__global__ __launch_bounds__(kThreads) void ps_map(const Item* __restrict__ items, float* dst, const float* src,
                                                   float divisor) {
  constexpr int PER = (int)(kSub / kBlkElems);
  const Item it = items[blockIdx.x / PER];
  const int64_t b0 = it.begin + (int64_t)(blockIdx.x % PER) * kBlkElems;
  const int64_t end = min(b0 + (int64_t)kBlkElems, it.end);
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = b0 + 4 * ((int64_t)k * kThreads + threadIdx.x);
    if (e >= end) continue;
    float4 t = src ? load_quad<false>(src, e, end) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (divisor != 0.0f) {
      t.x = t.x / divisor; t.y = t.y / divisor; t.z = t.z / divisor; t.w = t.w / divisor;
    }
    if (e + 4 <= end) {
      *reinterpret_cast<float4*>(dst + e) = t;
    } else {
      const float tj[3] = {t.x, t.y, t.z};
      for (int j = 0; j < 3 && e + j < end; ++j) dst[e + j] = tj[j];
    }
  }
}

// ---------------------------------------------------------------- host side

struct PsCall {
  omf_plan* p;
  EncArgs a;
  const float* acc;
  const void* const* q;
  const float* const* bnorm;
  float* sum_out;
  float* avg_out;
  float divisor;
  LevelScale lv{1};
  int32_t L_in, bits_in;
  int logd_in, logd_out;
  const int64_t* boff_in;
  const int64_t* boff_out;
  int bits_out;
  int32_t L_out;
  hipStream_t st;
};

template <int IN, int OUT, int N>
void launch_ps(const PsCall& c) {
  PsArgs<N> s{};
  for (int k = 0; k < N; ++k) {
    s.q[k] = c.q[k];
    s.bnorm[k] = c.bnorm[k];
  }
  s.acc = c.acc; s.sum_out = c.sum_out; s.avg_out = c.avg_out; s.boff_in = c.boff_in; s.divisor = c.divisor;
  s.levels = c.lv.levels; s.inv_levels = c.lv.inv_levels; s.L_in = c.L_in; s.bits_in = c.bits_in; s.logd_in = c.logd_in;
  const unsigned blocks = (unsigned)(c.p->n_flat * (kSub / kBlkElems));
  launch_kernel(qsgd_bucket_ps<IN, OUT, N>, dim3(blocks), dim3(kThreads), 0, c.st, c.a, s, c.boff_out, c.logd_out,
                c.bits_out, c.L_out, (int)c.p->bucket_pack);
}

template <int IN, int OUT>
void launch_ps_n(const PsCall& c, int n) {
  constexpr int MAX = IN == 1 ? kPsMaxI8 : (IN == 4 ? kPsMaxI32 : kPsMaxPacked);
  with_group_size<MAX>(n, [&](auto N) { launch_ps<IN, OUT, N()>(c); });
}

// n = 0 has no input wire: one instance per output.
template <int OUT>
void launch_ps_in(const PsCall& c, int width_in, int n) {
  if (n == 0) return launch_ps<1, OUT, 0>(c);
  if (width_in == 8) return launch_ps_n<1, OUT>(c, n);
  if (width_in == 32) return launch_ps_n<4, OUT>(c, n);
  launch_ps_n<0, OUT>(c, n);
}

void launch_map(const PsCall& c, float* dst, const float* src, float divisor) {
  if (dst == src && divisor == 0.0f) return;
  const unsigned blocks = (unsigned)(c.p->n_flat * (kSub / kBlkElems));
  hipLaunchKernelGGL(ps_map, dim3(blocks), dim3(kThreads), 0, c.st, (const Item*)c.p->d_flat, dst, src, divisor);
}

size_t payload_bytes(const omf_plan* p, int width, int bits) {
  if (width == 8) return (size_t)((p->arena_end + 3) & ~(int64_t)3);
  if (width == 32) return (size_t)p->arena_end * 4;
  return (size_t)((p->arena_end + 31) / 32) * (size_t)bits * 4;
}

}  // namespace

extern "C" {

int omf_ps_sum_encode_bucketed(omf_plan* p, const float* acc, const void* const* q_in, const float* const* bnorm_in,
                               int32_t nclients, int32_t width_in, int32_t levels_in, int64_t bucket_in, float* sum_out,
                               float divisor, float* avg_out, int32_t bit_width, int64_t bucket_out, int32_t pack_out,
                               uint64_t seed, uint64_t offset, void* q_out, float* bnorm_out, void* stream) {
  const std::string who = "omf_ps_sum_encode_bucketed: ";
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd_in = bucket::log2_size(bucket_in), logd_out = bucket::log2_size(bucket_out);
  if (logd_in < 0 || logd_out < 0) return fail(OMF_EINVAL, kBucketBadSize);
  if (bit_width < 0 || bit_width > 30) return fail(OMF_EINVAL, "bit_width must be in [0, 30] (levels = 2^bit_width is an int32 on the wire)");
  if (nclients < 0) return fail(OMF_EINVAL, who + "nclients must be >= 0");
  if (nclients == 0 && !acc) return fail(OMF_EINVAL, who + "no client and no accumulator");
  if (width_in != 8 && width_in != 32 && width_in != 0) return fail(OMF_EINVAL, "width_in must be 8, 32 or 0 (packed)");
  int32_t bits_in = 0;
  if (nclients > 0) {
    if (levels_in <= 0) return fail(OMF_EINVAL, "levels must be > 0");
    if (width_in == 0) {
      bits_in = omf_qsgd_packed_bits(levels_in);
      if (bits_in < 0 || bits_in > 32) return fail(OMF_EINVAL, "levels must be in [1, 2^31 - 1)");
    }
    if (!q_in || !bnorm_in) return fail(OMF_EINVAL, who + "q_in and bnorm_in must be non-NULL");
  }
  if (!avg_out || !q_out || !bnorm_out) return fail(OMF_EINVAL, who + "avg_out, q_out and bnorm_out must be non-NULL");
  const int32_t L_out = (int32_t)1 << bit_width;
  const int width_out = pack_out ? 0 : (L_out <= 127 ? 8 : 32);
  const int bits_out = omf_qsgd_packed_bits(L_out);  // bit_width + 2
  if ((acc && !aligned(acc, 16)) || (sum_out && !aligned(sum_out, 16)) || !aligned(avg_out, 16) || !aligned(bnorm_out, 4) ||
      !aligned(q_out, width_out == 8 ? 4 : (width_out == 32 ? 16 : 8)))
    return fail(OMF_EINVAL, kBucketMisaligned);
  const size_t ybytes = (size_t)p->arena_end * 4;
  if (acc && overlaps(avg_out, ybytes, acc, ybytes)) return fail(OMF_EINVAL, who + "avg_out overlaps acc");
  if (sum_out && overlaps(avg_out, ybytes, sum_out, ybytes)) return fail(OMF_EINVAL, who + "avg_out overlaps sum_out");
  if (sum_out && acc && sum_out != acc && overlaps(sum_out, ybytes, acc, ybytes))
    return fail(OMF_EINVAL, who + "sum_out must be acc itself or disjoint from it");
  const size_t qbytes = payload_bytes(p, width_in, bits_in);
  const size_t nbytes = (size_t)bucket::offsets(p->sizes.data(), p->nt, logd_in, nullptr) * 4;
  for (int32_t k = 0; k < nclients; ++k) {
    if (!q_in[k] || !bnorm_in[k]) return fail(OMF_EINVAL, who + "a NULL entry in q_in or bnorm_in");
    if (!aligned(q_in[k], width_in == 32 ? 16 : 4) || !aligned(bnorm_in[k], 4)) return fail(OMF_EINVAL, kBucketMisaligned);
    for (float* y : {avg_out, sum_out})
      if (y && (overlaps(y, ybytes, q_in[k], qbytes) || overlaps(y, ybytes, bnorm_in[k], nbytes)))
        return fail(OMF_EINVAL, who + "avg_out or sum_out overlaps a payload or norm buffer");
  }
  if (pack_out || (nclients > 0 && width_in == 0)) {  // offsets that are multiples of 32
    ArenaArgs arena;
    dim3 unused;
    if (const int rc = packed_arena(p, &arena, &unused)) return rc;
  }
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  DeviceGuard g(p->device);
  if (!g.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  PsCall c;
  c.p = p; c.st = (hipStream_t)stream;
  int64_t nb = 0;
  if (int r = bucket_tables(p, logd_in, &c.boff_in, &nb)) return r;
  if (int r = bucket_tables(p, logd_out, &c.boff_out, &nb)) return r;
  c.lv = LevelScale(nclients > 0 ? levels_in : 1);
  c.L_in = levels_in; c.bits_in = bits_in; c.logd_in = logd_in; c.logd_out = logd_out;
  c.bits_out = bits_out; c.L_out = L_out;

  // the clients of `n` payloads from k0 added onto `dst` (which holds the sum so far) by the existing sum kernels
  const auto sum_onto = [&](float* dst, int32_t k0, int32_t n) {
    if (width_in == 0)
      return omf_qsgd_decode_sum_bucketed_packed(p, reinterpret_cast<const uint32_t* const*>(q_in) + k0, bnorm_in + k0, n,
                                                 levels_in, bucket_in, dst, 1, 0.0f, stream);
    return omf_qsgd_decode_sum_bucketed(p, q_in + k0, bnorm_in + k0, n, width_in, levels_in, bucket_in, dst, 1, 0.0f, stream);
  };
  float* const part = sum_out ? sum_out : avg_out;  // where a partial sum is kept

  const bool fuse = (nclients == 0 || (c.lv.pow2 && bits_in <= 16)) && !(pack_out && bits_out > 16);
  if (!fuse) {  // the calls this one replaces, on the tensors' elements
    const float* sum = acc;
    if (nclients > 0) {
      launch_map(c, part, acc, 0.0f);
      OMF_HIP(hipGetLastError());
      if (int r = sum_onto(part, 0, nclients)) return r;
      sum = part;
    } else if (sum_out) {
      launch_map(c, sum_out, acc, 0.0f);
    }
    launch_map(c, avg_out, sum, divisor);
    OMF_HIP(hipGetLastError());
    if (pack_out)
      return omf_qsgd_encode_bucketed_packed(p, avg_out, 1.0f, bit_width, bucket_out, nullptr, seed, offset, nullptr,
                                             static_cast<uint32_t*>(q_out), bnorm_out, stream);
    return omf_qsgd_encode_bucketed(p, avg_out, 1.0f, bit_width, bucket_out, nullptr, seed, offset, nullptr, q_out,
                                    bnorm_out, stream);
  }

  const int32_t per = width_in == 8 ? kPsMaxI8 : (width_in == 32 ? kPsMaxI32 : (bits_in <= 8 ? kPsMaxPacked : kPsMaxPackedWide));
  const int32_t lead = nclients > per ? ((nclients - 1) / per) * per : 0;  // the leading groups' clients
  c.acc = acc;
  if (lead > 0) {
    launch_map(c, part, acc, 0.0f);
    OMF_HIP(hipGetLastError());
    if (int r = sum_onto(part, 0, lead)) return r;
    c.acc = part;  // avg_out itself without sum_out: every thread reads its quads before it writes them
  }
  c.q = q_in + lead; c.bnorm = bnorm_in + lead;
  c.sum_out = sum_out; c.avg_out = avg_out; c.divisor = divisor;
  c.a = enc_args(p, EncCall{nullptr, 1.0f, bit_width, nullptr, seed, offset, nullptr, q_out, bnorm_out, false, c.st, 0.0f,
                            nullptr, 0u, nullptr, width_out == 0 ? 0 : width_out / 8});
  c.a.items = p->d_flat;
  c.a.tinfo = p->d_tinfo[0];
  const int n = nclients - lead;
  if (width_out == 8) launch_ps_in<1>(c, width_in, n);
  else if (width_out == 32) launch_ps_in<4>(c, width_in, n);
  else launch_ps_in<0>(c, width_in, n);
  OMF_HIP(hipGetLastError());
  p->last_encoder = kEncBucketedPs;
  return OMF_OK;
}

}  // extern "C"
