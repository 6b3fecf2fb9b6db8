// omf_bracket.h — internal interface of the bracketed single-read QSGD encoder (omf_qsgd_bracket.hip).
//
// Not part of the C ABI: encode_launch (omf_qsgd.hip) hands a call that choose_encoder gave to the
// bracketed encoder to omf::bracket::launch.  What both units need of an encode call is here too: the
// call record, the kernel arguments every encoder takes from it, and the typed kernel launch.
// DESIGN.md §3.1 describes the algorithm.
#pragma once

#include <type_traits>

#include "omf_plan.h"
#include "omf_qsgd_enc.h"

namespace omf {

// The pass lists the quads it cannot decide in a slot per 4 Ki block; the plan's block holds the slots
// and records of the narrow capacity (upload_plan), and omf_plan_spec_stats counts the full lists.
constexpr int kSpecSlot = 32;     // words per block: 4 waves x 7 quads (+ 4 spare)
constexpr int kSpecPerWave = 7;   // listed quads per wave

// The fused PS step's last client (omf_ps_accumulate_apply_encode): its payload, width, level
// count and norms, and where acc + decode(q) goes (NULL: nowhere).
struct AccIn {
  const void* q;
  int32_t width, levels;
  const float* norm;
  float* acc_out;
};

// One encode call (the arguments of encode_impl) and its payload width in bytes.
struct EncCall {
  const float* x;
  float alpha;
  int32_t s;
  const float* u;
  uint64_t seed, offset;
  const float* norm_in;
  void* q;
  float* norm_out;
  bool norm_only;
  hipStream_t st;
  float divisor;
  float* xout;
  uint32_t fmt;
  const AccIn* acc_in;
  int width;
};

// Launches kernel `k` with exactly its parameter types (the caller checks hipGetLastError).
template <class... P>
void launch_kernel(void (*k)(P...), dim3 grid, dim3 blk, size_t lds, hipStream_t st, std::type_identity_t<P>... args) {
  void* params[] = {&args...};
  (void)hipLaunchKernel(reinterpret_cast<const void*>(k), grid, blk, params, lds, st);
}

// The buffers of a group made at the first encode that needs it (omf_qsgd.hip): the regions declared
// in `c`, each an allocation of its own that the plan owns; on failure every pointer of it is NULL.
// Hidden, as omf::bracket::launch is: calls between two units are not library exports.
__attribute__((visibility("hidden"))) int make_buffers(omf_plan* p, const plan_layout::Carve& c, hipStream_t st);

namespace bracket {

// The bracket, the pass and the finish of one encode on c.st; no host interaction.  0 or an OMF_E* code.
__attribute__((visibility("hidden"))) int launch(omf_plan* p, const EncCall& c, const plan_layout::Choice& ch);

}  // namespace bracket
}  // namespace omf

// What every encoder takes from the call; items, tinfo, epoch and n_items are the launcher's.
static inline EncArgs enc_args(const omf_plan* p, const omf::EncCall& c) {
  EncArgs a{};
  a.x = c.x; a.u = c.u; a.norm_in = c.norm_in; a.q = c.q; a.norm_out = c.norm_out;
  a.partials = p->d_partials;
  a.ticket = reinterpret_cast<uint32_t*>(p->d_sync);
  a.err = p->err_word();
  a.counters = reinterpret_cast<uint32_t*>(p->d_sync + p->off_counters);
  a.gran = reinterpret_cast<uint64_t*>(p->d_sync + p->off_gran);
  a.alpha = c.alpha;
  a.fmt = c.fmt;
  a.levels = (float)(1u << c.s);
  a.seed_lo = (uint32_t)c.seed; a.seed_hi = (uint32_t)(c.seed >> 32); a.offset = (uint32_t)c.offset;
  a.wait_ticks = p->wait_ticks;
  return a;
}
