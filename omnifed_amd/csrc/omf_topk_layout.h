// omf_topk_layout.h — the host-only side of Top-K: the constants host and kernels share, the
// per-tensor rules (k, bucket slots, sampling stride / runs / blocks, items, super-items) written
// once for both, the encoder's constant tables and pipeline groups, the carve of the encode and
// decode workspaces and of the plan-owned device tables, the decoder's tables, and the opt-in
// bit-packed index wire (its width rule, the group pack / unpack the kernels and the host check share,
// the packed arena's tables) with the quantised-value wire's layout rule beside it.
//
// Pure integer code: no HIP header, so tests/host/topk_layout_check.cpp runs it on a CPU under
// sanitizers.  omf_topk.hip (the encoder's host side) and omf_topk_recv.hip (decode and checks) upload what
// the builders return and bind their pointers with the carves declared here; the encoder's kernels
// (omf_topk_sampled.hip, omf_topk_exact.hip) and the receive kernels call the same rule functions.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "omf_plan_layout.h"

#ifdef __HIPCC__  // the rules below are the kernels' too
#define OMF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define OMF_HD inline
#endif

namespace omf {
namespace topk_layout {

// ---------------------------------------------------------------- constants
constexpr int kBins = 1024;   // exact path: histogram bins of the top 10 key bits, per tensor
constexpr int kSBits = 13;    // sample histogram: exponent + 5 mantissa bits
constexpr int kSBins = 1 << kSBits;
#ifndef OMF_SRUN  // experiment builds may override it (scripts/exp/tk_srun_ab.sh)
#define OMF_SRUN 16
#endif
constexpr int kSRun = OMF_SRUN;  // a sample is a 64-byte run of 16 consecutive elements,
constexpr int kSStride = 256;   // one run per >= 256 elements,
// default: at most 2 Ki runs (32 Ki samples) per tensor (OMF_TOPK_SAMPLE_RUNS).  Llama-400M encode:
// 1.024 ms at 2 Ki runs, 1.097 at 4 Ki, 1.142 at 8 Ki, 1.194 at 16 Ki (scripts/exp/tk_runs_sweep.py):
// the sample's random sectors cost more than the tighter threshold saves in the bucket kernels.
constexpr int kSMaxRuns = 2048;
// 2 Ki runs per sample block = one block per tensor at the default sample size: its LDS histogram is
// the tensor's, so it derives the threshold at once, with no global flush (Llama-400M: 54 -> 37 us
// against 512 runs per block, scripts/exp/tk_sblock_ab.sh); larger samples still split.
#ifndef OMF_SRUNS_PER_BLOCK  // experiment builds may override it
#define OMF_SRUNS_PER_BLOCK 2048
#endif
constexpr int kSRunsPerBlock = OMF_SRUNS_PER_BLOCK;
constexpr int64_t kSub = 16384;  // elements per flat item of the plan, which the Top-K kernels walk
static_assert(kSub == plan_layout::kSub, "the Top-K kernels walk the plan's flat items");
// Bucket sort of the candidates (the fast path): fine bins per tensor (<= kFineMax), buckets
// of whole fine bins whose rank starts fall in one kBucketHalf-wide window (so <= 2x that
// many keys when no fine bin exceeds kBucketHalf), each sorted in LDS by one block.
constexpr int kCoarse = 1024;    // coarse (sample-resolution) bins mapped per tensor
constexpr int kFineMax = 16384;  // fine bins per tensor
constexpr int kBucketHalf = 2048;
// A tensor's bucket-key region: k + kBucketPad keys (the k-th key's bin may run past rank k by up to
// one bucket's worth: a fine bin of up to 2 kBucketHalf keys sits in a bucket of its own).
constexpr int kBucketPad = 2 * kBucketHalf;
#ifndef OMF_TK_SUBPER  // experiment builds may override it
#define OMF_TK_SUBPER 512
#endif
constexpr int kSubPer = OMF_TK_SUBPER;               // elements per block of the fused pass
constexpr int kSubsPerItem = (int)(kSub / kSubPer);  // 32
constexpr int kSupItems = 1024 / kSubsPerItem;  // items per super-item (x 32 sub-chunks = 1024 runs)
constexpr int kZChunk = 2 * kSubPer;  // elements per zero-fill chunk (kThreads x 4)
constexpr uint32_t kScatterSmallB = 4096;  // most bucket slots of a tensor the LDS-table scatter kernels take
constexpr int kRadixDigits = 256;  // the exact tail's digit table: 4 kRadixDigits bytes per workgroup
// arena decode: super-tiles of 2^16 elements, kDecChunk selected values per place block
constexpr int kDecSuperBits = 16;
constexpr int kDecMaxSuper = 16384;  // LDS bins of a place block (arenas <= 2^30 elements)
constexpr int kDecChunk = 4096;      // selected values per place block
constexpr int kArenaMaxTensors = 4096;  // the arena decode's tensor lookup keeps koff in LDS

// One bucket of the fast path: its keys at bkeys[key_off, + count), its first rank `start`
// within the tensor; count | tensor << 16 (a bucket holds <= 2 kBucketHalf keys).
struct BucketRec {
  uint64_t key_off;
  uint32_t start;
  uint32_t count_tensor;
};

// ---------------------------------------------------------------- per-tensor rules (host and device)
// k = max(1, int(n * ratio)) (the reference's).
OMF_HD int64_t topk_k(int64_t n, double ratio) {
  const int64_t k = (int64_t)((double)n * ratio);
  return k < 1 ? 1 : k;
}
// Bucket slots of a tensor: the kBucketHalf-wide rank windows below k, plus one bucket of its own for
// each "big" fine bin (> kBucketHalf keys, topk_scatter_planned), at most k / (kBucketHalf + 1) + 1 of them.
OMF_HD uint32_t bucket_slots(int64_t k) { return (uint32_t)(2 * (k / kBucketHalf) + 3); }
// The sample: one run of kSRun elements per `stride` elements, at most max_runs runs, kSRunsPerBlock
// runs per sample block.
OMF_HD int64_t sample_stride(int64_t n, int64_t max_runs) {
  const int64_t s = (n + max_runs - 1) / max_runs;
  return s > (int64_t)kSStride ? s : (int64_t)kSStride;
}
OMF_HD int64_t sample_runs(int64_t n, int64_t stride) { return (n + stride - 1) / stride; }
OMF_HD uint32_t sample_blocks(int64_t runs) { return (uint32_t)((runs + kSRunsPerBlock - 1) / kSRunsPerBlock); }
// Flat items (kSub elements, as plan_layout::build_tables makes them) and super-items (kSupItems items).
OMF_HD int64_t tensor_items(int64_t n) { return (n + kSub - 1) / kSub; }
OMF_HD uint32_t tensor_supers(int64_t items) { return (uint32_t)((items + kSupItems - 1) / kSupItems); }

// ---------------------------------------------------------------- carve
// One allocation carved into kAlign-byte aligned regions in declaration order, each declared once with
// the member of S (a struct of typed pointers) that addresses it and its element count; bind() returns
// the pointers for a base address.  plan_layout::Carve's sibling: it fills a struct per call (callers'
// workspaces differ from call to call) instead of fields fixed at declaration.
constexpr size_t kAlign = 256;
inline size_t align256(size_t b) { return (b + kAlign - 1) & ~(kAlign - 1); }

template <class S>
class Carve {
 public:
  struct Region {
    const char* name;
    size_t offset, bytes;
    void (*set)(S& s, unsigned char* addr);
  };
  template <auto Member>
  void add(const char* name, size_t count) {
    using T = std::remove_pointer_t<std::remove_reference_t<decltype(std::declval<S&>().*Member)>>;
    regions_.push_back(Region{name, total_, sizeof(T) * count,
                              [](S& s, unsigned char* addr) { s.*Member = reinterpret_cast<T*>(addr); }});
    total_ = align256(total_ + sizeof(T) * count);
  }
  size_t bytes() const { return total_; }
  const std::vector<Region>& regions() const { return regions_; }
  S bind(void* base) const {
    S s{};
    for (const Region& r : regions_) r.set(s, static_cast<unsigned char*>(base) + r.offset);
    return s;
  }

 private:
  std::vector<Region> regions_;
  size_t total_ = 0;
};
#define OMF_REGION(carve, S, member, count) (carve).add<&S::member>(#member, (count))

// ---------------------------------------------------------------- encode tables
// Per (sizes, ratio, sample size): what the encoder's kernels read beside the plan's own tables.
struct EncodeTables {
  // per tensor (prefix sums carry their total at index nt)
  std::vector<int64_t> kk;      // k_t
  std::vector<int64_t> koff;    // [nt + 1] first value of the tensor's selection
  std::vector<int64_t> kb2;     // its bucket-key region: koff[t] + t * kBucketPad
  std::vector<uint32_t> tfirst, tlast;  // its flat items [tfirst, tlast]
  std::vector<uint32_t> bbase;  // [nt + 1] its bucket-table slots
  std::vector<uint32_t> sbase;  // [nt + 1] its super-items
  std::vector<uint32_t> smap;     // per sample block {tensor, first run}
  std::vector<uint32_t> supinfo;  // per super-item {tensor, first item, items, 1 on its tensor's first}
  std::vector<uint32_t> zmap;     // per zero-fill chunk {tensor, chunk}: the kZChunk chunks below index k_t
  int32_t nsb = 0, nzb = 0;       // sample blocks, zero-fill chunks
  // host only: what make_groups sums
  std::vector<int64_t> sizes;
  std::vector<uint32_t> sblk;   // [nt + 1] the tensor's sample blocks
};
EncodeTables build_encode_tables(const std::vector<int64_t>& sizes, double ratio, int64_t max_runs);

// Pipeline groups of the sampled path: contiguous tensor ranges of about equal element counts.
struct Group {
  int32_t t0 = 0, t1 = 0;                           // tensors [t0, t1)
  uint32_t sb0 = 0, nsb = 0, sub0 = 0, nsub = 0;    // sample blocks, fused-pass blocks
  uint32_t sup0 = 0, nsup = 0, bk0 = 0, nbk = 0;    // super-items, bucket slots
  uint32_t nb_max = 0;                              // most bucket slots of one tensor
};
std::vector<Group> make_groups(const EncodeTables& tb, int G);

// The plan-owned device table of one EncodeTables: its vectors, the sample histograms gh / zero
// counts gz and the arrival counters of the sample (per tensor) and plan kernels — zeroed once
// ([zero_begin, bytes) of the table), left zeroed by every call.
struct SetupTable {
  int64_t *kk, *koff, *kb2;
  uint32_t *tfirst, *tlast, *bbase, *sbase, *smap, *supinfo, *zmap, *done, *arrive, *gz, *gh;
};
struct SetupCarve {
  Carve<SetupTable> carve;
  size_t zero_begin = 0;
};
SetupCarve setup_table_carve(const EncodeTables& tb);

// The latest tables of a plan, host and device side (keyed by the ratio's bits and the sample size).
struct EncodeSetup {
  bool valid = false;
  uint64_t ratio_bits = 0;
  int64_t max_runs = 0;
  EncodeTables host;
  SetupTable dev{};
};

// ---------------------------------------------------------------- encode workspace
struct EncodeWs {
  uint32_t *hist, *bin, *cnt, *flag, *status;  // the zeroed prefix
  uint32_t *tkey, *zcnt, *seg_b, *seg_e;
  int64_t* cstart;
  uint32_t *sub_cnt, *item_cnt, *item_off;
  uint64_t *cand, *sorted;
  uint32_t *fmap, *tlo, *thi, *fcount, *fhist;
  int32_t* fbucket;
  uint32_t* bstart;
  BucketRec* brec;
  uint32_t* bfill;
  unsigned char* tmp;
};
// The caller's workspace of an arena.  Everything below zero_end is cleared once per call on the exact
// path; the sampled path clears its redo histograms in topk_sample and writes the rest.  tmp_bytes:
// the exact tail's digit table (4 kRadixDigits bytes per CU) or the library sort's temporary.
struct EncodeWsLayout {
  Carve<EncodeWs> carve;
  size_t zero_end = 0, tmp_bytes = 0, total = 0;
  size_t nb_max = 0;  // bucket-table slots for any ratio (k <= n)
};
EncodeWsLayout encode_ws_layout(const std::vector<int64_t>& sizes, int64_t arena_end, size_t tmp_bytes);

// ---------------------------------------------------------------- decode
inline int32_t dec_nsuper(int64_t arena_end) {
  return (int32_t)((arena_end + (1 << kDecSuperBits) - 1) >> kDecSuperBits);
}
inline int64_t dec_place_blocks(int64_t ktot) { return std::max<int64_t>(1, (ktot + kDecChunk - 1) / kDecChunk); }

// The tiled decode's tables of the selection layout ks (per-tensor counts): koff[nt + 1] (each tensor's
// first value), cap_base[nsuper + 1] (the bucket-capacity prefix: 2 x the expected count of the
// super-tile, each tensor's k spread over its elements, + 256, at most a super-tile's elements) and
// blk_t (per place block: its first and last tensor, the largest t with koff[t] <= j).
struct DecodeTables {
  std::vector<int64_t> koff;
  std::vector<uint32_t> cap_base, blk_t;
  int32_t nsuper = 0;
};
DecodeTables dec_tables_host(const std::vector<int64_t>& sizes, const std::vector<int64_t>& offsets,
                             int64_t arena_end, const int64_t* ks);

// The plan-owned device table of one DecodeTables.
struct DecTable {
  int64_t* koff;
  uint32_t *cap_base, *blk_t;
};
Carve<DecTable> dec_table_carve(int32_t nt, int32_t nsuper, int64_t place_blocks);

// Caller workspace of the tiled zero-fill decode: fill[nsuper] + the overflow count (left zero by
// every call), the buckets (cap_total entries) and the overflow list (ktot).
struct DecWs {
  uint32_t* fill;
  uint64_t *pairs, *ovf;
};
Carve<DecWs> dec_ws_layout(int32_t nsuper, uint64_t cap_total, int64_t ktot);

// ---------------------------------------------------------------- bit-packed indices (opt-in wire)
// "TopKBitPackedCompression": the k tensor-local indices of a tensor of n elements in
// b = index_bits(n) bits each, LSB-first little-endian — index i at bits [i b, (i + 1) b) of the tensor's
// stream.  In a packed arena 32 consecutive indices of one tensor (a group; a tensor's last one may be
// partial) are exactly b words and start on a word; tensor t's first group is goff[t], its first word woff[t].
constexpr int kPackGroup = 32;
constexpr int64_t kPackMaxElems = (int64_t)1 << 32;  // b <= 32

// b = max(1, bit_length(n - 1)); -1 outside [1, 2^32].
OMF_HD int32_t index_bits(int64_t n) {
  if (n < 1 || n > kPackMaxElems) return -1;
  int32_t b = 1;
  while (b < 32 && ((int64_t)1 << b) < n) ++b;
  return b;
}

// One group: the low b bits of idx[0, nv) and code 0 for the rest of the 32, into the b words out[0, b)
// (T: the index wire's int64 indices, the value wire's 32-bit codes).
template <class T>
OMF_HD void pack_group(const T* idx, int nv, int b, uint32_t* out) {
  const uint64_t mask = (1ull << b) - 1ull;
  uint64_t acc = 0;
  int nb = 0, w = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int i = 0; i < kPackGroup; ++i) {
    const uint64_t code = i < nv ? (uint64_t)idx[i] & mask : 0ull;
    acc |= code << nb;  // nb < 32 and code < 2^32: no bit is lost
    nb += b;
    if (nb >= 32) {
      out[w++] = (uint32_t)acc;
      acc >>= 32;
      nb -= 32;
    }
  }
}

// The first nv codes of a group's words w[0, b), zero-extended into out[0, nv).  Only the words that
// hold one of those codes are read, and of the last of them only the codes' bits are used: whatever
// lies past bit nv * b does not matter.
template <class T>
OMF_HD void unpack_group(const uint32_t* w, int nv, int b, T* out) {
  const uint64_t mask = (1ull << b) - 1ull;
  uint64_t acc = 0;
  int nb = 0, wi = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int i = 0; i < kPackGroup; ++i) {
    if (i < nv) {
      if (nb < b) {
        acc |= (uint64_t)w[wi++] << nb;
        nb += 32;
      }
      out[i] = (T)(acc & mask);
      acc >>= b;
      nb -= b;
    }
  }
}

// The packed arena of the selection layout ks over `sizes`: per tensor its width, first group
// goff[t] = sum_{u<t} ceil(k_u / 32) and first word woff[t] = sum_{u<t} ceil(k_u / 32) b_u (both with
// their totals at index nt), koff as the decode tables'.  words = woff[nt], or -1 when a tensor is
// outside index_bits' range (its bits entry is -1 and it adds no words).
struct PackTables {
  std::vector<int32_t> bits;
  std::vector<int64_t> koff, goff, woff;
  int64_t words = 0;
};
PackTables pack_tables_host(const std::vector<int64_t>& sizes, const int64_t* ks);

// The plan-owned device table of one PackTables (goff as 32-bit words: the callers refuse 2^32 groups).
struct PackTable {
  int64_t *koff, *woff;
  uint32_t* goff;
  int32_t* bits;
};
Carve<PackTable> pack_table_carve(int32_t nt);

// ---------------------------------------------------------------- quantised values (opt-in wire)
// "TopKQuantPackedCompression": the k selected values of a tensor as QSGD levels q in [-L, L], L = 2^s,
// against the tensor's scale max |v|; code q + L in b = s + 2 bits, packed as the indices are: value i
// at bits [i b, (i + 1) b) of the tensor's stream, a group of 32 consecutive values of one tensor in b
// whole words.  b is the same for every tensor, so group g of the selection (g = goff[t] + j for tensor
// t's j-th group: the index wire's goff) starts at word g b and the value arena holds goff[nt] b words.
constexpr int kQvalMinBits = 1, kQvalMaxBits = 8;  // s

// b = s + 2 = bit_length(2 L) (the packed QSGD wire's width for L levels); -1 outside s = 1..8.
OMF_HD int32_t value_code_bits(int32_t s) { return s >= kQvalMinBits && s <= kQvalMaxBits ? s + 2 : -1; }
OMF_HD int64_t value_group_word(int64_t g, int32_t b) { return g * (int64_t)b; }
inline int64_t value_words(const PackTables& p, int32_t b) { return value_group_word(p.goff.back(), b); }

}  // namespace topk_layout
}  // namespace omf
