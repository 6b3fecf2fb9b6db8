// omf_qsgd_bucket_ps_max.hip — the parameter server's step for max-scaled bucketed QSGD, with or without the
// Hadamard rotation, MI355X (gfx950): K clients' payloads decoded, summed in client order, taken back from the
// rotated domain, added to the accumulator, divided and re-encoded against each bucket's max |z| in ONE launch in
// which the average never returns from HBM, with its host side (omf_ps_sum_encode_bucketed_max).  DESIGN.md §3.4h.
// The rules of the scale and the transform are omf_qsgd_bucket_rot.h's, the blocks and the transform of a block
// its shared steps (block_of, rotate_block, load_levels), the draws, the level math and the payload stores the
// encoders' (quant_rows, store_quad), the decode rule the decoders' (dec_quad).
//
// Kernel map:
//   qsgd_bucket_ps_max<WIDTH_IN, WIDTH_OUT, N, ROT, REQ>   the work split of omf_qsgd_bucket_rot.hip: one 256-thread
//                    workgroup per block of 4 rows (4096 elements) of a flat 16 Ki item, row k of thread tid the quad
//                    at 4 (k 256 + tid) of the block, one bucket size for both directions.
//                    Front half, every global load issued before the first use: per row the N clients' quads of
//                    levels and their buckets' scales, the quad the sum starts from and (ROT) the accumulator's.
//                    The sum runs in registers in client order, __fadd_rn from the start (or +0), in the domain the
//                    levels were taken in: sum_block's sum.  A launch with `part_out` stores it there and stops
//                    (the leading groups of a call of more clients than one launch takes).
//                    REQ = 0: (ROT) the inverse transform, then acc + sum; the store to sum_out; / divisor; +0 past
//                    the block's end; the non-temporal store to avg_out; (ROT) the forward transform of the average,
//                    through the same 16 KiB LDS tile after a barrier; max |z| per bucket on the bit patterns
//                    (bucket_maxes), stored by the bucket's first lane; quant_rows with store_quad.
//                    REQ = 1 (ROT, no accumulator): the downlink first, from W = Z / divisor with Z the sum still
//                    in the rotated domain — H_d H_d = d I, so W is the forward transform of the average up to
//                    rounding and no forward butterfly runs — then the inverse, sum_out, the division and avg_out
//                    as above.  A short last bucket is never rotated: there W is the average itself.
//                    N, the clients of the launch, is a template parameter (exact-N instances; N = 0: the
//                    accumulator alone, no transform back); the bucket size is a kernel argument.  From d <= 256
//                    no transform touches LDS.  No workgroup waits for another: no polling, no ticket, no atomic.
//
// Not HBM-bound with the rotation on; no MFMA (the bit rules fix the butterfly's adds).
#include <string>

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

// Clients per launch, from the registers the gfx950 build reports: N quads of levels and N
// scales per row are in flight with two arenas' quads and the sum.
constexpr int kPsMaxI8 = 8, kPsMaxI32 = 4;

template <int N>
struct PsMaxArgs {
  const void* q[N ? N : 1];       // client c's payload arena
  const float* scale[N ? N : 1];  // its scale arena
  const float* start;             // what the sum starts from, in the sum's own domain, or NULL: +0
  const float* acc;               // ROT: added to the sum once it is back from the rotated domain, or NULL
  float* part_out;                // non-NULL: the sum is stored here as it is and the launch ends
  float* sum_out;                 // NULL: the sum is not stored
  float* avg_out;
  float divisor;                  // 0: no division
  float levels, inv_levels;       // fl32(L_in) and 2^-s_in (0: L_in is no power of two)
};

// z += the N clients' decodes, in client order; lanes past the block's end keep +0 (sum_block's loop, the loads
// already made).
template <int WIDTH_IN, bool POW2, int N, bool FULL>
__device__ __forceinline__ void add_clients(float (&z)[kRows][4], const int32_t (&raw)[N ? N : 1][kRows][4],
                                            const float (&sc)[N ? N : 1][kRows], float levels, float inv_levels,
                                            const Blk& bk) {
#pragma unroll
  for (int c = 0; c < N; ++c) {
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
      const bool live = FULL || bk.b + 4 * ((int64_t)k * kThreads + threadIdx.x) < bk.end;
      float yv[4];
      dec_quad<WIDTH_IN, POW2>(raw[c][k], sc[c][k], levels, inv_levels, yv);
#pragma unroll
      for (int j = 0; j < 4; ++j) z[k][j] = live ? __fadd_rn(z[k][j], yv[j]) : 0.0f;
    }
  }
}

// The downlink of a block's values w (+0 past the block's end): max |w| per bucket, the scale's store, the levels.
template <int WIDTH_OUT, bool FULL>
__device__ __forceinline__ void encode_rows(const float (&w)[kRows][4], const EncArgs& a, const Blk& bk, int64_t nbase,
                                            int logd, uint32_t (*xch)[kWaves]) {
  uint32_t m[kRows];
  float4 v[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const uint32_t abs = 0x7FFFFFFFu;
    m[k] = max(max(__float_as_uint(w[k][0]) & abs, __float_as_uint(w[k][1]) & abs),
               max(__float_as_uint(w[k][2]) & abs, __float_as_uint(w[k][3]) & abs));
    v[k] = make_float4(w[k][0], w[k][1], w[k][2], w[k][3]);
  }
  bucket_rot::bucket_maxes(m, logd, xch);
  float norm[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) norm[k] = __uint_as_float(m[k]);
  bucket_norms_store<FULL, kRows>(a.norm_out, bk.b, bk.end, bk.tbegin, nbase, logd, norm);
  quant_rows<false, FULL, kRows>(v, a, bk.b, bk.end, bk.tbegin, bk.tensor, norm,
                                 [&](int, int64_t e, const int32_t (&qq)[4]) { store_quad<WIDTH_OUT, FULL>(a, e, bk.end, qq); });
}

// w = z / divisor (0: z), +0 at every element past the block's end.
template <bool FULL>
__device__ __forceinline__ void divide_rows(const float (&z)[kRows][4], float divisor, const Blk& bk, float (&w)[kRows][4]) {
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = bk.b + 4 * ((int64_t)k * kThreads + threadIdx.x);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[k][j] = divisor != 0.0f ? z[k][j] / divisor : z[k][j];
      if (!FULL && e + j >= bk.end) w[k][j] = 0.0f;
    }
  }
}

template <bool FULL>
__device__ __forceinline__ void store_rows(float* y, const float (&z)[kRows][4], const Blk& bk) {
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = bk.b + 4 * ((int64_t)k * kThreads + threadIdx.x);
    if (FULL || e < bk.end) store_f4<FULL>(y, e, bk.end, z[k]);
  }
}

template <int WIDTH_IN, int WIDTH_OUT, int N, bool ROT, bool REQ, bool FULL>
__device__ __forceinline__ void ps_max_block(const EncArgs& a, const PsMaxArgs<N>& s, const RotGeom& g, const Blk& bk,
                                             float4* tile, uint32_t (*xch)[kWaves]) {
  constexpr int NC = N ? N : 1;
  const int tid = (int)threadIdx.x, logd = g.logd;
  const int64_t rel = (bk.b - bk.tbegin) + 4 * tid, nbase = g.boff[bk.tensor];
  // ---- every global load
  int32_t raw[NC][kRows][4];
  float sc[NC][kRows];
  float4 s0[kRows], p[kRows];
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const int64_t e = bk.b + 4 * ((int64_t)k * kThreads + tid);
    const bool live = FULL || e < bk.end;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      load_levels<WIDTH_IN, FULL>(s.q[c], e, bk.end, raw[c][k]);
      sc[c][k] = live ? s.scale[c][nbase + ((rel + 1024 * k) >> logd)] : 0.0f;
    }
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s0[k] = s.start ? load_quad<FULL, true>(s.start, e, bk.end) : zero;
    p[k] = (ROT && s.acc) ? load_quad<FULL, true>(s.acc, e, bk.end) : zero;
  }
  // ---- the sum, in client order
  float z[kRows][4];
#pragma unroll
  for (int k = 0; k < kRows; ++k) { z[k][0] = s0[k].x; z[k][1] = s0[k].y; z[k][2] = s0[k].z; z[k][3] = s0[k].w; }
  if (N > 0) {
    if (s.inv_levels != 0.0f) add_clients<WIDTH_IN, true, N, FULL>(z, raw, sc, s.levels, s.inv_levels, bk);
    else add_clients<WIDTH_IN, false, N, FULL>(z, raw, sc, s.levels, s.inv_levels, bk);
  }
  if (s.part_out) {  // uniform: a leading group
    store_rows<FULL>(s.part_out, z, bk);
    return;
  }
  float w[kRows][4];
  if (REQ) {  // the downlink from the rotated domain
    divide_rows<FULL>(z, s.divisor, bk, w);
    encode_rows<WIDTH_OUT, FULL>(w, a, bk, nbase, logd, xch);
  }
  if (ROT && N > 0) {
    rotate_block<true, FULL>(z, g, bk, logd, tile);
    if (s.acc) {
#pragma unroll
      for (int k = 0; k < kRows; ++k) {
        z[k][0] = __fadd_rn(p[k].x, z[k][0]); z[k][1] = __fadd_rn(p[k].y, z[k][1]);
        z[k][2] = __fadd_rn(p[k].z, z[k][2]); z[k][3] = __fadd_rn(p[k].w, z[k][3]);
      }
    }
  }
  if (s.sum_out) store_rows<FULL>(s.sum_out, z, bk);
  divide_rows<FULL>(z, s.divisor, bk, w);
  store_rows<FULL>(s.avg_out, w, bk);
  if (REQ) return;
  if (ROT) {
    if (N > 0 && logd >= 9) __syncthreads();  // the tile: the inverse's reads before the forward's writes
    rotate_block<false, FULL>(w, g, bk, logd, tile);
  }
  encode_rows<WIDTH_OUT, FULL>(w, a, bk, nbase, logd, xch);
}

// WIDTH_IN / WIDTH_OUT: 1 int8, 4 int32.  a: the output side as the encoders take it (q, norm_out, levels, the
// Philox key; alpha = 1, no x, u or norm_in).
template <int WIDTH_IN, int WIDTH_OUT, int N, bool ROT, bool REQ>
__global__ __launch_bounds__(kThreads) void qsgd_bucket_ps_max(EncArgs a, PsMaxArgs<N> s, RotGeom g) {
  static_assert(!REQ || (ROT && N > 0), "the rotated-domain downlink needs rotated clients");
  __shared__ float4 tile[ROT ? bucket_rot::kTileQuads : 1];
  __shared__ uint32_t xch[kRows][kWaves];
  const Blk bk = block_of(g);
  if (bk.b >= bk.end) return;
  if (bk.end - bk.b == kBlk) ps_max_block<WIDTH_IN, WIDTH_OUT, N, ROT, REQ, true>(a, s, g, bk, tile, xch);
  else ps_max_block<WIDTH_IN, WIDTH_OUT, N, ROT, REQ, false>(a, s, g, bk, tile, xch);
}

// ---------------------------------------------------------------- host side

struct PsMaxCall {
  omf_plan* p;
  EncArgs a;
  RotGeom g;
  LevelScale lv{1};
  bool int32_out, rot, req;
  hipStream_t st;
};

// One launch over clients [q, q + N): the sum from `start`, then stored to part_out, or carried to the end.
struct PsMaxStep {
  const void* const* q;
  const float* const* scale;
  const float* start;
  const float* acc;
  float* part_out;
  float* sum_out;
  float* avg_out;
  float divisor;
};

template <int WIDTH_IN, int N>
void launch_ps_max(const PsMaxCall& c, const PsMaxStep& t) {
  PsMaxArgs<N> s{};
  for (int k = 0; k < N; ++k) {
    s.q[k] = t.q[k];
    s.scale[k] = t.scale[k];
  }
  s.start = t.start; s.acc = t.acc; s.part_out = t.part_out; s.sum_out = t.sum_out; s.avg_out = t.avg_out;
  s.divisor = t.divisor; s.levels = c.lv.levels; s.inv_levels = c.lv.inv_levels;
  const auto go = [&](auto kern) { launch_kernel(kern, dim3(rot_grid_blocks(c.p)), dim3(kThreads), 0, c.st, c.a, s, c.g); };
  const auto out = [&](auto W) {
    constexpr int WO = decltype(W)::value;
    if (!c.rot) return go(qsgd_bucket_ps_max<WIDTH_IN, WO, N, false, false>);
    if constexpr (N > 0) {
      if (c.req) return go(qsgd_bucket_ps_max<WIDTH_IN, WO, N, true, true>);
    }
    go(qsgd_bucket_ps_max<WIDTH_IN, WO, N, true, false>);
  };
  if (c.int32_out) out(std::integral_constant<int, 4>{});
  else out(std::integral_constant<int, 1>{});
}

// n = 0 has no input wire: one instance per output.
void launch_ps_max_n(const PsMaxCall& c, const PsMaxStep& t, int width_in, int n) {
  if (n == 0) return launch_ps_max<1, 0>(c, t);
  if (width_in == 8) return with_group_size<kPsMaxI8>(n, [&](auto N) { launch_ps_max<1, N()>(c, t); });
  with_group_size<kPsMaxI32>(n, [&](auto N) { launch_ps_max<4, N()>(c, t); });
}

}  // namespace

extern "C" {

int omf_ps_sum_encode_bucketed_max(omf_plan* p, const float* acc, const void* const* q_in, const float* const* bnorm_in,
                                   int32_t nclients, int32_t width_in, int32_t levels_in, int64_t bucket_size,
                                   int32_t rotate, uint32_t rot_seed, int32_t tensor_keyed, int32_t requantise_rotated,
                                   float* sum_out, float divisor, float* avg_out, int32_t bit_width, uint64_t seed,
                                   uint64_t offset, void* q_out, float* bnorm_out, void* stream) {
  const std::string who = "omf_ps_sum_encode_bucketed_max: ";
  if (!p) return fail(OMF_EINVAL, "plan is NULL");
  const int logd = bucket::log2_size(bucket_size);
  if (logd < 0) return fail(OMF_EINVAL, kBucketBadSize);
  if (bit_width < 0 || bit_width > 30) return fail(OMF_EINVAL, "bit_width must be in [0, 30] (levels = 2^bit_width is an int32 on the wire)");
  if (nclients < 0) return fail(OMF_EINVAL, who + "nclients must be >= 0");
  if (nclients == 0 && !acc) return fail(OMF_EINVAL, who + "no client and no accumulator");
  if (width_in != 8 && width_in != 32) return fail(OMF_EINVAL, "width_in must be 8 or 32");
  if (requantise_rotated && (!rotate || acc))
    return fail(OMF_EINVAL, who + "requantise_rotated needs rotate and no accumulator");
  if (nclients > 0) {
    if (levels_in <= 0) return fail(OMF_EINVAL, "levels must be > 0");
    if (!q_in || !bnorm_in) return fail(OMF_EINVAL, who + "q_in and bnorm_in must be non-NULL");
  }
  if (!avg_out || !q_out || !bnorm_out) return fail(OMF_EINVAL, who + "avg_out, q_out and bnorm_out must be non-NULL");
  const bool int32_out = ((int32_t)1 << bit_width) > 127;
  if ((acc && !aligned(acc, 16)) || (sum_out && !aligned(sum_out, 16)) || !aligned(avg_out, 16) || !aligned(bnorm_out, 4) ||
      !aligned(q_out, int32_out ? 16 : 4))
    return fail(OMF_EINVAL, kBucketMisaligned);
  const size_t ybytes = (size_t)p->arena_end * 4;
  if (acc && overlaps(avg_out, ybytes, acc, ybytes)) return fail(OMF_EINVAL, who + "avg_out overlaps acc");
  if (sum_out && overlaps(avg_out, ybytes, sum_out, ybytes)) return fail(OMF_EINVAL, who + "avg_out overlaps sum_out");
  if (sum_out && acc && sum_out != acc && overlaps(sum_out, ybytes, acc, ybytes))
    return fail(OMF_EINVAL, who + "sum_out must be acc itself or disjoint from it");
  const size_t qbytes = width_in == 8 ? (size_t)((p->arena_end + 3) & ~(int64_t)3) : ybytes;
  const size_t nbytes = (size_t)bucket::offsets(p->sizes.data(), p->nt, logd, nullptr) * 4;
  for (int32_t k = 0; k < nclients; ++k) {
    if (!q_in[k] || !bnorm_in[k]) return fail(OMF_EINVAL, who + "a NULL entry in q_in or bnorm_in");
    if (!aligned(q_in[k], width_in == 32 ? 16 : 4) || !aligned(bnorm_in[k], 4)) return fail(OMF_EINVAL, kBucketMisaligned);
    for (float* y : {avg_out, sum_out})
      if (y && (overlaps(y, ybytes, q_in[k], qbytes) || overlaps(y, ybytes, bnorm_in[k], nbytes)))
        return fail(OMF_EINVAL, who + "avg_out or sum_out overlaps a payload or norm buffer");
  }
  if (!p->d_block) return fail(OMF_EHIP, "the plan's tables are not on the device (an earlier upload failed)");
  DeviceGuard dg(p->device);
  if (!dg.ok) return fail(OMF_EHIP, "hipSetDevice failed");
  PsMaxCall c;
  c.p = p; c.st = (hipStream_t)stream; c.int32_out = int32_out; c.rot = rotate != 0; c.req = requantise_rotated != 0;
  if (int r = rot_geom(p, logd, rot_seed, tensor_keyed, &c.g)) return r;
  c.lv = LevelScale(nclients > 0 ? levels_in : 1);
  c.a = enc_args(p, EncCall{nullptr, 1.0f, bit_width, nullptr, seed, offset, nullptr, q_out, bnorm_out, false, c.st, 0.0f,
                            nullptr, 0u, nullptr, int32_out ? 4 : 1});

  const int32_t per = width_in == 8 ? kPsMaxI8 : kPsMaxI32;
  float* const part = sum_out ? sum_out : avg_out;  // where a partial sum is kept: every thread reads its quads
  PsMaxStep t{};                                    // of it before it writes them
  t.sum_out = sum_out; t.avg_out = avg_out; t.divisor = divisor;
  int32_t k0 = 0;
  if (c.rot && acc && nclients > per) {
    // omf_qsgd_decode_sum_bucketed_rot onto a copy of acc inverts each of its groups (kBucketSumMax clients) and
    // adds it in turn: its own launches for the leading groups, and for a last group that exceeds one launch here
    const int32_t last = nclients - ((nclients - 1) / kBucketSumMax) * kBucketSumMax;
    k0 = last <= per ? nclients - last : nclients;
    if (part != acc) {
      PsMaxStep m{};
      m.start = acc; m.part_out = part;
      launch_ps_max_n(c, m, width_in, 0);
      OMF_HIP(hipGetLastError());
    }
    if (int r = omf_qsgd_decode_sum_bucketed_rot(p, q_in, bnorm_in, k0, width_in, levels_in, bucket_size, rot_seed,
                                                 tensor_keyed, part, 1, 0.0f, stream))
      return r;
    if (k0 < nclients) t.acc = part;
    else t.start = part;  // the sum is whole: the accumulator alone
  } else {
    // one client-order sum in the sum's own domain: from acc (no rotation), or from +0 with acc added after the
    // one inverse; the leading groups leave it in `part`
    t.start = c.rot ? nullptr : acc;
    t.acc = c.rot ? acc : nullptr;
    for (; nclients - k0 > per; k0 += per) {
      PsMaxStep m = t;
      m.q = q_in + k0; m.scale = bnorm_in + k0; m.acc = nullptr; m.part_out = part;
      launch_ps_max_n(c, m, width_in, per);
      OMF_HIP(hipGetLastError());
      t.start = part;
    }
    if (nclients == 0) { t.start = acc; t.acc = nullptr; }
  }
  t.q = q_in + k0; t.scale = bnorm_in + k0;
  launch_ps_max_n(c, t, width_in, nclients - k0);
  OMF_HIP(hipGetLastError());
  p->last_encoder = kEncBucketedPsMax;
  return OMF_OK;
}

}  // extern "C"
