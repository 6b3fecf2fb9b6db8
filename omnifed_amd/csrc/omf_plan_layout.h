// omf_plan_layout.h — the host-only side of a QSGD plan: the table record types the kernels read,
// the layout constants they depend on, the builders of every work-item table, the carve of the
// plan's one device allocation, and the choice of the encoder that serves a call.
//
// Pure integer code: no HIP header, so tests/host/plan_layout_check.cpp runs it on a CPU under
// sanitizers.  omf_qsgd.hip uploads what build_tables returns and launches what choose_encoder picks
// (the bracketed encoder through omf_bracket.h, the ring through omf_ring.h).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace omf {

// ---------------------------------------------------------------- single-read ring (omf_qsgd_ring.hip)
namespace ring {

// Work-item flags: a chunk publishes its partial sum of squares and/or quantises.
//   kPublish | kQuant  HOLD   read once: partial, keep the chunk on chip, quantise later
//   kPublish           NORM   partial only (first pass of a tensor too large to hold)
//   kQuant             QUANT  second pass of such a tensor: re-read and quantise
enum : int32_t { kPublish = 1, kQuant = 2 };

// 64 bytes = one scalar load: the tensor's fields ride along so the hot loops never make
// a second, dependent table read.
struct Item {
  int64_t begin, end;    // arena element range (one chunk of one tensor)
  int64_t tbegin, tn;    // the tensor's range
  int32_t tensor, flags, chunk, nchunks;
  int32_t gbase, pad[3];  // the tensor's first granule
};

struct Tensor {
  int64_t begin, n;
  int32_t nchunks, gbase;  // partial granules of this tensor: gran[gbase .. gbase + nchunks)
  int32_t pad[2];
};

}  // namespace ring

namespace plan_layout {

// ---------------------------------------------------------------- constants
constexpr int kBlkWaves = 4;         // wave partials per 4 Ki block: one per wave of a 256-thread workgroup
constexpr int64_t kSub = 16384;      // elements per flat item = 64 KiB fp32 (16 float4 per thread)
constexpr int64_t kSpecBlk = 4096;   // elements per block of the bracketed pass (4 float4 per thread)
constexpr int64_t kDecBlk = 4096;    // elements per block of the decoder's table
constexpr int kSpecSeg = 4096;       // wave partials per fold workgroup (16 loads per thread in flight: a
                                     // 4 Mi-element tensor is one segment)
constexpr int kSpecRun = 64;         // elements per sampled run (256 B: DRAM-friendly)
constexpr int kSpecRuns = 512;       // sampled runs per larger tensor (at most)
// wide levels: 4x the sampled elements (half the bracket width: the undecided quads, the fix pass's
// work, grow with L and with the bracket's width) in runs of 256 elements (1 KiB: four times fewer
// random DRAM accesses than 2 Ki runs of 64), kBrParts workgroups per tensor, 128 runs each
constexpr int kSpecRunWide = 256;
constexpr int kSpecRunsWide = 512;
#ifndef OMF_BR_PARTS  // experiment builds may override it (scripts/exp/s8_variants.sh)
#define OMF_BR_PARTS 2
#endif
constexpr int kBrParts = OMF_BR_PARTS;
constexpr int kFbParts = 8;  // fused bracket: 64 runs each, four float4 per thread (the pass's blocks' register budget)
#ifndef OMF_WFB_PARTS  // experiment builds may override it
#define OMF_WFB_PARTS 16
#endif
constexpr int kWfbParts = OMF_WFB_PARTS;  // wide fused bracket: one-wave parts per tensor
constexpr int kGridNB = 3;  // grid encoder: 4 Ki blocks per quarter-workgroup per launch
// Level counts the bracketed encoder serves.  The undecided fraction grows with L (a level step is
// norm / L wide): at L = 32 a 1 Mi-element tensor's sampled bracket already leaves ~1.3 undecided
// quads per wave, so bit widths 5-8 take the wide-level lists (fp32 only).
constexpr int kSpecMinBits = 1;  // L >= 2 (spec_check.c's underflow argument)
constexpr int kSpecMaxBits = 4;
constexpr int kSpecMaxBitsWide = 8;
static_assert(kSub == 4 * kSpecBlk, "four spec blocks per flat item");

// ---------------------------------------------------------------- table records
enum : int32_t { kNorm = 0, kQuant = 1, kResident = 2 };

struct Item {
  int64_t begin, end;  // arena element range of this work item
  int32_t tensor, kind, chunk, pad;
};

struct TensorInfo {
  int64_t begin, n;
  int64_t chunk;          // elements per item of this tensor
  int32_t nchunks, pbase;
};

// Bracket work item: one per tensor, one workgroup each (qsgd_spec_bracket writes the
// tensor's bracket from that workgroup's sums alone; build_tables makes exactly one).
struct SpecBrItem {
  int64_t begin, n;  // the tensor's arena range
  int64_t base;      // stratum length n / R (R = runs of the tensor); rem = n % R strata are one longer
  int32_t R, rem;
  int32_t tensor, Rw;  // Rw: the runs of kSpecRunWide sampled for wide levels (strata n / Rw)
};
// Fold work item: wave partials [p_begin, p_end) of tensor `tensor`, segment `seg` of `nsegs`.
struct SpecFoldItem {
  int64_t p_begin, p_end;
  int32_t tensor, seg, nsegs, sbase;
};

// ---------------------------------------------------------------- tables
// What the tables depend on: the arena, the two-pass encoder's shape and the ring's.
struct Desc {
  const int64_t* sizes = nullptr;    // per tensor, > 0
  const int64_t* offsets = nullptr;  // ordered, non-overlapping
  int32_t nt = 0;
  int64_t chunk = 2 * kSub;    // two-pass encode items (a multiple of kSub)
  int32_t ev = 8;              // encode rows per thread: resident items of ev * 1024 elements
  int64_t cap = 1;             // tensors of <= cap resident items take the register-resident path
  int64_t ring_chunk = kSub;   // the ring configuration: chunk elements, slots, kind (omf_ring.h Config)
  int32_t ring_slots = 1, ring_kind = 0;
  int32_t ring_grid = 1;       // co-resident workgroups of a ring launch
  int32_t ring_big_mode = 1;   // 0: QUANT chunks of a large tensor ring_gap items after its NORM chunks; 1: NORM first, QUANT last
  int64_t ring_gap = -1;       // items (-1: one grid)
  int64_t ring_hold_override = 0;  // > 0: hold limit in chunks (tests)
};

struct Tables {
  std::vector<Item> enc[2];          // ticket-order sequences: [0] register-resident + two-pass, [1] two-pass
  std::vector<TensorInfo> tinfo[2];
  std::vector<Item> flat;            // one kSub item each: decode, norm-supplied quantise, Top-K, the bracketed pass
  std::vector<ring::Item> ring;
  std::vector<ring::Tensor> ring_t;
  std::vector<SpecBrItem> br_items;      // one per tensor
  std::vector<SpecFoldItem> fold_items;  // segments of kSpecSeg wave partials
  std::vector<uint32_t> grid_pbeg, grid_pcnt;  // grid encoder, per tensor: first flat item, flat items
  std::vector<uint32_t> dec_binfo;   // per kDecBlk block: tensor id | (1 << 31 when the block lies inside it)
  int64_t n_enc[2] = {0, 0}, n_flat = 0;
  int64_t n_partials = 0;            // fp64 partials of the larger ticket-order sequence (>= 1)
  int64_t n_spec_blocks = 0;         // 4 Ki blocks: 4 per flat item
  int64_t n_ring_gran = 0;           // ring granules, one per chunk (>= 1)
  int64_t ring_hold_max = 0;         // tensors of more ring chunks are read twice
  int64_t ring_two_pass = 0;         // how many are
};

// Builds every host table of `d`; false if the arena makes more work items than an int32 counts.
bool build_tables(const Desc& d, Tables& out);

// ---------------------------------------------------------------- device allocation
inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// One allocation, carved into 16-byte aligned regions in declaration order.  A region is declared
// once, with the pointer that will address it, its element count and its initial contents; the
// declarations give the allocation's size, and bind() the pointers.
class Carve {
 public:
  struct Region {
    size_t offset, bytes;
    const void* src;  // host contents to upload (NULL: none)
    bool zero;        // fill with zero bytes
    void* field;      // the T* that addresses the region
    void (*set)(void* field, void* addr);
  };
  template <class T>
  void copy(T*& field, const std::vector<T>& host) { add(field, host.size(), host.data(), false); }
  template <class T>
  void copy(T*& field, const T* host, size_t count) { add(field, count, host, false); }
  template <class T>
  void zero(T*& field, size_t count) { add(field, count, static_cast<const T*>(nullptr), true); }
  template <class T>
  void raw(T*& field, size_t count) { add(field, count, static_cast<const T*>(nullptr), false); }  // written before it is read
  size_t bytes() const { return total_; }
  const std::vector<Region>& regions() const { return regions_; }
  // Points every declared pointer at its region of the allocation at `base`; NULL clears them all.
  void bind(void* base) const {
    for (const Region& r : regions_) r.set(r.field, base ? static_cast<unsigned char*>(base) + r.offset : nullptr);
  }

 private:
  template <class T>
  void add(T*& field, size_t count, const T* src, bool zero) {
    regions_.push_back(Region{total_, sizeof(T) * count, src, zero, &field,
                              [](void* f, void* a) { *static_cast<T**>(f) = static_cast<T*>(a); }});
    total_ = round16(total_ + sizeof(T) * count);
  }
  std::vector<Region> regions_;
  size_t total_ = 0;
};

// ---------------------------------------------------------------- encoder choice
// The encoders, numbered as omf_plan_last_encoder reports them (0-4 are also the strategies).
enum Encoder : int32_t {
  kEncResident = 0,     // ticket-ordered launch: register-resident small tensors + two-pass
  kEncOrdered = 1,      // ticket-ordered launch: two-pass everywhere
  kEncRing = 2,         // single-read ring
  kEncBracket = 3,      // bracketed single-read
  kEncGrid = 4,         // one-launch grid encoder
  kEncCallerNorms = 5,  // levels with caller norms: one pass, no hand-off
};

struct Call {
  int32_t strategy = 2;        // the plan's (omf_plan_set_encode_strategy)
  int32_t bits = 0;            // bit width s
  bool caller_u = false;       // uniforms supplied
  bool caller_norms = false;   // norms supplied
  bool norms_only = false;
  uint32_t fmt = 0;            // value format: 0 fp32, 1 bf16, 2 fp16
  bool divide = false;         // fused PS step
  bool last_client = false;    // fused last client's decode-accumulate
  bool wide_levels = true;     // omf_plan_set_wide_levels
  bool fused_bracket = true;   // omf_plan_set_fused_bracket
  uint32_t spec_dbg = 0;       // omf_plan_set_debug spec bits (bit 0: no bracket launch)
  bool grid_fits = false;      // the arena fits one launch of the grid encoder
};

struct Choice {
  Encoder encoder;
  // kEncBracket only: wide levels (bit widths 5-8); the bracket folded into the pass launch (else
  // it is a launch of its own, unless spec_dbg bit 0 skips it)
  bool wide = false, fused = false, bracket_launch = false;
};

// A norms-only pass always runs the ticket-ordered launch (kEncOrdered's tables unless the
// strategy is 0) and does not count as the plan's last encoder.
Choice choose_encoder(const Call& c);

}  // namespace plan_layout
}  // namespace omf
