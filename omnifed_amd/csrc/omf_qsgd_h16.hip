// omf_qsgd_h16.hip — QSGD encode of bf16 / fp16 tensors from a 16-bit arena, MI355X (gfx950).
//
// The other encoders read an fp32 arena, so a 16-bit model's update is first upcast into one: 2 B read
// and 4 B written per element before the encoder's 4 B read and 1 B written.  Here the arena holds the
// tensors' own 16-bit patterns at the plan's element offsets, and the values are widened in registers:
//   qsgd_h16_sumsq   one workgroup per item of the two-pass sequence (NORM items and the single items of
//                    small tensors; QUANT items leave at once): the item's sum of squares with the
//                    two-pass encoder's accumulation order — thread tid's row k of a sub-chunk at b is the
//                    quad at b + 4 (k kThreads + tid), one fp32 fma chain per thread over the item, the
//                    block's fp64 sum — and the ticketed fold of omf_qsgd_enc.h, whose last arriver writes
//                    the tensor's norm to norm_out.  The norm's bits are the two-pass encoder's on the
//                    exact fp32 upcast.
//   qsgd_h16_quant   after it on the stream (so no in-kernel wait): V * 1024-element blocks of the flat
//                    16 Ki items, values re-read with non-temporal loads, weighted, quantised with the
//                    norm from norm_out (or the caller's) and stored — quant_store of omf_qsgd_enc.h, the
//                    element math of every encoder.
// 2 + 2 + 1 = 5 bytes per element on the int8 wire, against 11 through the upcast.
//
// Loads (load_h4, omf_qsgd_enc.h): a thread's quad is 8 bytes, one 8-byte load per lane and row.  The WIDE
// kernels load 16 bytes per lane, two adjacent quads of one row, and swap the foreign quad with the
// neighbouring lane by DPP, so the thread -> quad mapping (and with it the norm's order, the Philox slots
// and the payload stores) stays the shared one; they need every tensor to start on a 16-byte boundary
// (offsets that are multiples of 8).  Measured slower (Llama-400M bf16: 0.477 against 0.467 ms at 4 rows per
// block, 0.509 against 0.485 at 8; profiles/h16_encode_ab.json), so they run only when omf_plan_set_h16 asks.
// HBM-bound; no MFMA (no contraction).
#include "omf_h16.h"

using namespace omf;
using namespace omf::plan_layout;

namespace {

// One thread's fp32 sum of squares over [b, e): sub-chunks of EV rows in order (chunk_sumsq's order).
template <int EV, bool WIDE, bool BF16>
__device__ __forceinline__ float h16_sumsq(const EncArgs& a, const uint16_t* __restrict__ x, int64_t b, int64_t e) {
  constexpr int64_t S = (int64_t)EV * 1024;
  float acc = 0.0f;
  for (int64_t sb = b; sb < e; sb += S) {
    const int64_t se = min(sb + S, e);
    float4 v[EV];
    // default cache policy: the quantise launch's re-read may hit the Infinity Cache
    if (se - sb == S) load_h4<EV, true, false, WIDE, BF16>(x, sb, se, v);
    else load_h4<EV, false, false, WIDE, BF16>(x, sb, se, v);
    scale_f4<EV>(v, a);
    acc = sumsq_f4<EV>(v, acc);
  }
  return acc;
}

template <int EV, bool WIDE>
__global__ __launch_bounds__(kThreads) void qsgd_h16_sumsq(EncArgs a, const uint16_t* __restrict__ x16) {
  __shared__ HandoffShared sh;
  const Item it = a.items[blockIdx.x];
  if (it.kind == kQuant) return;
  const TensorInfo ti = a.tinfo[it.tensor];
  const float acc = a.fmt == kFmtBF16 ? h16_sumsq<EV, WIDE, true>(a, x16, it.begin, it.end)
                                      : h16_sumsq<EV, WIDE, false>(a, x16, it.begin, it.end);
  publish_partial(a, ti, it.tensor, it.chunk, acc, sh);
}

// Load + scale + quantise + store the block [b, e) of V rows.
template <int WIDTH, bool HAS_U, int V, bool WIDE, bool BF16>
__device__ __forceinline__ void h16_quant_block(const EncArgs& a, const uint16_t* __restrict__ x, int64_t b,
                                                int64_t e, int64_t tbegin, int32_t tensor, float norm) {
  float4 v[V];
  if (e - b == (int64_t)V * 1024) {
    load_h4<V, true, true, WIDE, BF16>(x, b, e, v);
    scale_f4<V>(v, a);
    quant_store<WIDTH, HAS_U, true, V>(v, a, b, e, tbegin, tensor, norm);
  } else {
    load_h4<V, false, true, WIDE, BF16>(x, b, e, v);
    scale_f4<V>(v, a);
    quant_store<WIDTH, HAS_U, false, V>(v, a, b, e, tbegin, tensor, norm);
  }
}

// kSub / (V * 1024) blocks per flat item.  a.norm_in: the norms (norm_out itself after qsgd_h16_sumsq).
template <int WIDTH, bool HAS_U, int V, bool WIDE>
__global__ __launch_bounds__(kThreads) void qsgd_h16_quant(EncArgs a, const uint16_t* __restrict__ x16) {
  constexpr int PER = (int)(kSub / ((int64_t)V * 1024));
  const Item it = a.items[blockIdx.x / PER];
  const int64_t b = it.begin + (int64_t)(blockIdx.x % PER) * V * 1024;
  if (b >= it.end) return;
  const int64_t e = min(b + (int64_t)V * 1024, it.end);
  const int64_t tbegin = a.tinfo[it.tensor].begin;
  const float norm = a.norm_in[it.tensor];
  if (a.norm_in != a.norm_out && it.chunk == 0 && blockIdx.x % PER == 0 && threadIdx.x == 0) a.norm_out[it.tensor] = norm;
  if (a.fmt == kFmtBF16) h16_quant_block<WIDTH, HAS_U, V, WIDE, true>(a, x16, b, e, tbegin, it.tensor, norm);
  else h16_quant_block<WIDTH, HAS_U, V, WIDE, false>(a, x16, b, e, tbegin, it.tensor, norm);
}

using H16Kernel = void (*)(EncArgs, const uint16_t*);

}  // namespace

int omf::h16::launch(omf_plan* p, const EncCall& c, const void* x16) {
  static const H16Kernel sumsq[2][2] = {  // [16 rows per thread][16-byte loads]
      {qsgd_h16_sumsq<8, false>, qsgd_h16_sumsq<8, true>}, {qsgd_h16_sumsq<16, false>, qsgd_h16_sumsq<16, true>}};
  static const H16Kernel quant[2][2][2][2] = {  // [8 rows per block][int32 wire][caller uniforms][16-byte loads]
      {{{qsgd_h16_quant<1, false, 4, false>, qsgd_h16_quant<1, false, 4, true>},
        {qsgd_h16_quant<1, true, 4, false>, qsgd_h16_quant<1, true, 4, true>}},
       {{qsgd_h16_quant<4, false, 4, false>, qsgd_h16_quant<4, false, 4, true>},
        {qsgd_h16_quant<4, true, 4, false>, qsgd_h16_quant<4, true, 4, true>}}},
      {{{qsgd_h16_quant<1, false, 8, false>, qsgd_h16_quant<1, false, 8, true>},
        {qsgd_h16_quant<1, true, 8, false>, qsgd_h16_quant<1, true, 8, true>}},
       {{qsgd_h16_quant<4, false, 8, false>, qsgd_h16_quant<4, false, 8, true>},
        {qsgd_h16_quant<4, true, 8, false>, qsgd_h16_quant<4, true, 8, true>}}}};
  const uint16_t* x = static_cast<const uint16_t*>(x16);
  const bool wide = p->h16_wide != 0 && p->h16_aligned;
  EncArgs a = enc_args(p, c);
  if (!c.norm_in) {
    // As the ticket-ordered launch: no per-call memset (the arrival counters are reset in-kernel by their
    // last user), and the granules carry this launch's epoch.
    if (++p->epoch == 0) ++p->epoch;
    a.epoch = p->epoch;
    a.n_items = (uint32_t)p->n_enc[1];
    a.items = p->d_enc[1];
    a.tinfo = p->d_tinfo[1];
    launch_kernel(sumsq[p->ev != 8][wide], dim3((unsigned)p->n_enc[1]), dim3(kThreads), 0, c.st, a, x);
    OMF_HIP(hipGetLastError());
    a.norm_in = c.norm_out;
  }
  if (c.norm_only) return OMF_OK;
  const int rows = p->h16_rows == 8 ? 8 : 4;
  a.items = p->d_flat;
  a.tinfo = p->d_tinfo[0];
  const unsigned blocks = (unsigned)(p->n_flat * (kSub / (rows * 1024)));
  launch_kernel(quant[rows == 8][c.width == 4][c.u != nullptr][wide], dim3(blocks), dim3(kThreads), 0, c.st, a, x);
  OMF_HIP(hipGetLastError());
  return OMF_OK;
}
