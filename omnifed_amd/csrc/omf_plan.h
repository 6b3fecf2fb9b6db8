// omf_plan.h — internal definition of the plan behind the C ABI's opaque omf_plan.
//
// Not part of the C ABI.  omf_qsgd.hip creates, uploads and destroys a plan and launches the QSGD
// encoders from it (the bracketed encoder's: omf_qsgd_bracket.hip, which also makes that encoder's lazy
// buffers); omf_qsgd_recv.hip (the decoders and the K-client sum), omf_qsgd_pack.hip (the packed wire) and
// the Top-K units (omf_topk.hip the encoder's host side, omf_topk_sampled.hip and omf_topk_exact.hip its
// kernels and launches, omf_topk_recv.hip decode and checks, omf_topk_tie.hip the tie rewrite) read its arena
// tables; the Top-K units keep their per-plan device tables in it.  The host tables come from omf_plan_layout.h;
// Top-K's host state (its workspace layout, made at the plan's first Top-K use, and its latest encode tables)
// is omf_topk_layout.h's.
#pragma once

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/omf_codec.h"
#include "omf_common.h"
#include "omf_plan_layout.h"
#include "omf_topk_layout.h"

namespace omf {

constexpr uint64_t kWaitTicks = 2000000ull;  // 20 ms of the 100 MHz realtime clock

// A tensor's bracket of the bracketed encoder (written by its bracket workgroups).
struct SpecBracket {
  float c_lo, c_hi, n_lo, n_hi;
  uint32_t mode;  // 0 speculate, 1 deferred (degenerate sample: the fix pass requantises)
  uint32_t pad[3];
};

}  // namespace omf

struct omf_plan {
  int device = 0;
  int32_t nt = 0;
  int64_t chunk = omf::plan_layout::kSub;
  std::vector<int64_t> sizes, offsets;
  int64_t arena_end = 0;
  int64_t cap = 0;               // tensors of <= cap items take the register-resident path
  int32_t strategy = 2;          // 0 register-resident + two-pass, 1 ticket-ordered two-pass, 2 single-read ring,
                                 // 3 bracketed single-read (default by size: omf_plan_create), 4 grid
  int32_t last_encoder = -1;     // the encoder the latest encode launched (plan_layout::Encoder; omf_plan_last_encoder)
  uint64_t wait_ticks = omf::kWaitTicks;      // norm waits (ring: expiry recomputes; bracketed fix: expiry fails)
  uint64_t lds_wait_ticks = omf::kWaitTicks;  // the ring's on-chip hand-off waits (expiry aborts the workgroup)
  uint32_t epoch = 0;            // last granule tag used (host-side launch counter)
  int32_t ev = 8;                // encode rows per thread (sub-chunk = ev * 1024 elements): 8 measured
                                 // faster than 16 for the two-pass encoder (0.596 vs 0.606 ms, Llama-400M)
  // ---- the plan's block: one device allocation, carved by upload_plan (omf_qsgd.hip) in this order
  void* d_block = nullptr;
  uint8_t* d_sync = nullptr;    // [ticket u32, err u32, pad 8][counters u32 x nt, pad16][granules u64 x nt, pad16]
  size_t sync_bytes = 0, off_counters = 16, off_gran = 0;
  int64_t n_enc[2] = {0, 0};
  omf::plan_layout::Item* d_enc[2] = {nullptr, nullptr};
  int64_t n_flat = 0, n_partials = 0;
  omf::plan_layout::Item* d_flat = nullptr;
  omf::plan_layout::TensorInfo* d_tinfo[2] = {nullptr, nullptr};
  uint64_t* d_partials = nullptr;
  int64_t* d_sizes = nullptr;   // per-tensor element counts (Top-K)
  int64_t* d_begins = nullptr;  // per-tensor arena offsets (Top-K)
  // single-read ("ring") encoder, strategy 2 (omf_qsgd_ring.hip)
  int32_t ring_cfg = 0;         // omf_qsgd_ring.hip kConfigs[0]: 64 KiB chunks, 8 loader + 8 quantiser waves
  int32_t ring_grid = 0;
  int32_t ring_big_mode = 1;     // 0: QUANT chunks of a large tensor ring_gap items after its NORM chunks; 1: NORM first, QUANT last
  int64_t ring_gap = -1;         // items (-1: one grid)
  int64_t ring_hold_override = 0;  // > 0: hold limit in chunks (tests)
  uint32_t ring_dbg = 0;           // test / experiment switches (omf_plan_set_debug), 0 in production
  uint32_t ring_epoch = 0;
  int64_t n_ring = 0, n_ring_gran = 0, ring_hold_max = 0, ring_two_pass = 0;
  omf::ring::Item* d_ring = nullptr;
  omf::ring::Tensor* d_ring_t = nullptr;
  uint64_t* d_ring_gran = nullptr;
  unsigned long long* d_ring_prof = nullptr;  // 16 phase counters (OMF_RING_DBG & 4)
  // bracketed single-read encoder, strategy 3: per-tensor brackets / flags / status, per
  // 4 Ki-element block partials and undecided-quad slots
  int64_t n_spec_blocks = 0, n_spec_fold = 0;
  omf::plan_layout::SpecBrItem* d_spec_br_items = nullptr;  // one per tensor
  omf::plan_layout::SpecFoldItem* d_spec_fold_items = nullptr;
  uint64_t* d_spec_seg_part = nullptr;
  uint32_t* d_spec_cnt = nullptr;  // fold_cnt x nt
  omf::SpecBracket* d_spec_br = nullptr;
  uint64_t* d_spec_ngran = nullptr;  // per tensor {epoch << 1 | bad, norm} granules of the fold
  uint64_t* d_spec_part = nullptr;
  uint32_t* d_spec_slots = nullptr;
  uint32_t* d_spec_heads = nullptr;
  // arena-aligned decoder: per 4 Ki block, tensor id | (1 << 31 when inside it)
  int64_t n_dec_blocks = 0;
  uint32_t* d_dec_binfo = nullptr;
  float4* d_spec_recs = nullptr;  // listed quads' x and draws (32 B each)
  uint32_t* d_spec_flags = nullptr;
  uint32_t* d_spec_status = nullptr;
  // grid encoder (strategy 4): one workgroup per CU, kGridNB 4 Ki blocks per quarter
  int32_t grid_wgs = 0;             // workgroups of a launch (CUs; 0 = unavailable)
  uint32_t* d_grid_pbeg = nullptr;  // per tensor: first flat item (one partial per item)
  uint32_t* d_grid_pcnt = nullptr;  // per tensor: flat items
  unsigned long long* d_grid_bar = nullptr;  // arrival counter (zeroed at upload)
  uint64_t grid_launches = 0;
  // ---- the bracketed encoder's host state
  uint32_t spec_epoch = 0;
  uint32_t spec_skip = 0;  // test / experiment switches (omf_plan_set_debug), 0 in production
  // The bracket's width in sigmas (OMF_SPEC_ZSIG overrides both): a tensor whose norm falls
  // outside is requantised whole by the finish (exact; a miss per tensor at z sigmas has
  // probability ~erfc(z / sqrt 2): 6e-5 at 4, 6e-7 at 5), and a narrower bracket lists fewer
  // undecided quads.  scripts/exp/zsig_ab.sh, Llama-400M, two interleaved rounds: s = 4 encode
  // 0.349-0.352 ms at 5 sigmas against 0.357-0.361 at 6 (4: 0.350); s = 8 0.546-0.547 ms at 4
  // against 0.556-0.559 at 5 (3.5: 0.542-0.545).
  float spec_zsig = 5.0f;
  float spec_zsig_wide = 4.0f;
  // the fused-bracket pass (OMF_SPEC_FB=0 / omf_plan_set_fused_bracket turn it off): Llama-400M s = 4
  // step 0.6977-0.7021 ms against 0.7009-0.7067 with the bracket's own launch (three interleaved
  // pairs), the encode alone unchanged (0.348-0.360 both); profiles/r05_fused_bracket_ab.txt
  int32_t spec_fb = 1;
  int32_t spec_wide = 1;  // wide levels (5-8 bits, fp32) through the bracket (1) or as before (0): OMF_SPEC_WIDE
  int32_t spec_last_pw = 0;  // the list capacity of the latest bracketed encode
  // ---- buffers made at the first encode that needs them (ensure_wide / ensure_fused_bracket in
  // omf_qsgd_bracket.hip, through make_buffers of omf_qsgd.hip): all of a group's pointers are set or
  // none; d_lazy owns the allocations
  std::vector<void*> d_lazy;
  uint32_t* d_spec_slots_w = nullptr;  // wide levels (bit widths 5-8): slots and records of the wide
  float4* d_spec_recs_w = nullptr;     // list capacity,
  double* d_spec_br_part = nullptr;    // the bracket parts' partial sums and arrival counters
  uint32_t* d_spec_br_cnt = nullptr;
  double* d_spec_fb_part = nullptr;    // fused bracket: its parts' partial sums, arrival counters
  uint32_t* d_spec_fb_cnt = nullptr;   // and granules
  uint64_t* d_spec_brgran = nullptr;
  // Top-K tiled decode: per-ratio constant tables (omf_topk_recv.hip), allocated on first use, with
  // one host word each (the table's size facts)
  struct TopkTable {
    uint64_t key;
    void* dev;
    uint64_t host;
    std::vector<int64_t> counts;  // tables keyed by explicit per-tensor counts: the exact counts
  };
  std::vector<TopkTable> topk_tables;
  omf::TopkKnobs topk_knobs;
  // Top-K encode: the caller workspace's layout (omf_topk.hip encode_ws; the size query takes a
  // const plan) and the tables of the latest (ratio, sample size)
  mutable std::once_flag topk_ws_once;
  mutable omf::topk_layout::EncodeWsLayout topk_ws;
  omf::topk_layout::EncodeSetup topk_setup;
  // Launches that use the sync block / granules are ordered across streams: a launch on a
  // stream other than the previous one first waits for the previous launch's event.
  hipEvent_t last_ev = nullptr;
  hipStream_t last_stream = nullptr;
  bool last_valid = false;

  // The plan's device error word (omf_plan_check reports and clears it).
  uint32_t* err_word() const { return reinterpret_cast<uint32_t*>(d_sync + 4); }
};

namespace omf {

// Order this launch after the plan's previous stateful launch when the stream changes: the event is
// recorded on the previous stream at the switch (it covers everything enqueued there so far, the
// plan's launches included), not after every call — an event packet between two kernels of one
// stream idled the GPU ~5 us per encode even without a system-scope fence (rocprofv3 kernel trace).
// So the previous stream must still exist when the plan moves to another one (include/omf_codec.h).
inline int plan_enter(omf_plan* p, hipStream_t st) {
  if (p->last_valid && p->last_stream != st) {
    if (!p->last_ev) OMF_HIP(hipEventCreateWithFlags(&p->last_ev, kOrderEventFlags));
    OMF_HIP(hipEventRecord(p->last_ev, p->last_stream));
    OMF_HIP(hipStreamWaitEvent(st, p->last_ev, 0));
  }
  return OMF_OK;
}
inline int plan_leave(omf_plan* p, hipStream_t st) {
  p->last_stream = st;
  p->last_valid = true;
  return OMF_OK;
}

// A plan-owned device buffer of `bytes` for `key` (allocated, and *fresh set, on first use;
// not on the hot path after that), with a host word the caller keeps beside it.  nullptr if
// the allocation fails.
inline void* topk_table(omf_plan* p, uint64_t key, size_t bytes, bool* fresh, uint64_t** host) {
  *fresh = false;
  for (auto& e : p->topk_tables)
    if (e.key == key) {
      *host = &e.host;
      return e.dev;
    }
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
  p->topk_tables.push_back({key, d, 0, {}});
  *host = &p->topk_tables.back().host;
  *fresh = true;
  return d;
}
// The same for tables keyed by an explicit per-tensor count vector (a received Top-K message's
// k_t): matched on the kind and the exact counts.  At most kMaxCountTables of a kind are kept; making
// one more frees the oldest (hipFree waits for the device, so no queued launch still reads it).
constexpr uint64_t kCountsKey = 0xC0C0C0C0C0C0C0C0ull;      // the decode tables of a count vector
constexpr uint64_t kPackCountsKey = 0xC0C0C0C0C0C0B175ull;  // its packed-index tables (kept 8 of each kind)
inline void* topk_table_counts(omf_plan* p, const int64_t* counts, size_t bytes, bool* fresh, uint64_t** host,
                               uint64_t kind = kCountsKey) {
  constexpr int kMaxCountTables = 8;
  *fresh = false;
  const size_t nt = (size_t)p->nt;
  int held = 0;
  for (auto& e : p->topk_tables) {
    if (e.key != kind) continue;
    ++held;
    if (e.counts.size() == nt && std::equal(e.counts.begin(), e.counts.end(), counts)) {
      *host = &e.host;
      return e.dev;
    }
  }
  if (held >= kMaxCountTables) {
    for (auto it = p->topk_tables.begin(); it != p->topk_tables.end(); ++it)
      if (it->key == kind) {
        (void)hipFree(it->dev);
        p->topk_tables.erase(it);
        break;
      }
  }
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
  p->topk_tables.push_back({kind, d, 0, std::vector<int64_t>(counts, counts + nt)});
  *host = &p->topk_tables.back().host;
  *fresh = true;
  return d;
}

// 0 <= counts[t] <= sizes[t] for every tensor, *ktot their sum; else OMF_EINVAL (omf_topk_recv.hip).
int topk_check_counts(const omf_plan* plan, const int64_t* counts, int64_t* ktot);

// The plan's device tables of the packed wires for `counts` (koff, goff, the index wire's woff and bits;
// uploaded on first use) and the host facts a call needs: the selection's values, its 32-value groups and
// the index arena's words (omf_topk_pack.hip).  ktot = 0: no table, nothing to launch.
struct PackArgs {
  topk_layout::PackTable dev{};
  int64_t ktot = 0, groups = 0, words = 0;
};
int topk_pack_args(omf_plan* plan, const int64_t* counts, PackArgs* out);

}  // namespace omf
