// plan_layout_check.cpp — stand-alone CPU checker of omnifed_amd/csrc/omf_plan_layout.{h,cpp}
// (tests/test_plan_layout_host.py builds it with the sanitizers and runs it).
//
//   plan_layout_check [choice_table.txt]
//
// Builds every host table of a set of tiny arenas under every ring configuration kind, both big
// modes, three gaps and both rows-per-thread settings and checks the invariants the kernels rely on;
// checks the carve of a device allocation; and checks choose_encoder against the rows of the table
// file (written by the test from tests/golden/encoder_choice_parent.npz) and, over the full input
// space, against the properties that tie the uncovered inputs to the covered ones.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../omnifed_amd/csrc/omf_plan_layout.h"

using namespace omf::plan_layout;
namespace R = omf::ring;

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (++g_fail <= 20) std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
    }                                                                                    \
  } while (0)

using Ranges = std::vector<std::pair<int64_t, int64_t>>;

// [b, e) is covered by the ranges exactly once
static bool tiles(Ranges r, int64_t b, int64_t e) {
  std::sort(r.begin(), r.end());
  int64_t at = b;
  for (const auto& x : r) {
    if (x.first != at || x.second <= x.first) return false;
    at = x.second;
  }
  return at == e;
}

struct Arena {
  std::vector<int64_t> sizes, offsets;
  explicit Arena(std::vector<int64_t> s) : sizes(std::move(s)) {
    int64_t o = 0;
    for (int64_t n : sizes) {  // codec.arena_layout: tensors start on multiples of 64 elements
      offsets.push_back(o);
      o = (o + n + 63) / 64 * 64;
    }
  }
  int32_t nt() const { return (int32_t)sizes.size(); }
  int64_t end() const { return offsets.back() + sizes.back(); }
};

// A ticket-order sequence: coverage, NORM before QUANT, the partial bases.
static int64_t check_enc(const Arena& a, const Desc& d, const std::vector<Item>& seq, const std::vector<TensorInfo>& ti,
                         bool resident_ok) {
  const int32_t nt = a.nt();
  CHECK((int32_t)ti.size() == nt);
  std::vector<Ranges> quant(nt), publish(nt);
  std::vector<int64_t> last_norm(nt, -1), first_quant(nt, -1);
  for (size_t i = 0; i < seq.size(); ++i) {
    const Item& it = seq[i];
    CHECK(it.tensor >= 0 && it.tensor < nt);
    if (it.tensor < 0 || it.tensor >= nt) continue;
    const int32_t t = it.tensor;
    CHECK(it.kind == kNorm || it.kind == kQuant || it.kind == kResident);
    CHECK(it.begin == ti[t].begin + (int64_t)it.chunk * ti[t].chunk);
    CHECK(it.end == std::min(ti[t].begin + ti[t].n, it.begin + ti[t].chunk));
    if (it.kind != kNorm) quant[t].emplace_back(it.begin, it.end);
    if (it.kind != kQuant) publish[t].emplace_back(it.begin, it.end);
    if (it.kind == kNorm) last_norm[t] = (int64_t)i;
    if (it.kind == kQuant && first_quant[t] < 0) first_quant[t] = (int64_t)i;
  }
  int64_t pbase = 0;
  const int64_t es = (int64_t)d.ev * 1024;
  for (int32_t t = 0; t < nt; ++t) {
    const int64_t b = a.offsets[t], n = a.sizes[t];
    CHECK(ti[t].begin == b && ti[t].n == n);
    CHECK(tiles(quant[t], b, b + n));
    CHECK(tiles(publish[t], b, b + n));
    CHECK((last_norm[t] < 0) == (first_quant[t] < 0));
    CHECK(last_norm[t] < 0 || last_norm[t] < first_quant[t]);
    const int64_t ns = (n + es - 1) / es;
    const bool resident = ns == 1 || (resident_ok && ns <= d.cap);  // the rule of the two paths
    CHECK(resident == (last_norm[t] < 0));
    CHECK(ti[t].chunk == (resident ? es : d.chunk));
    CHECK(ti[t].pbase == pbase && ti[t].nchunks == (int32_t)publish[t].size());  // disjoint, in order
    pbase += ti[t].nchunks;
  }
  return pbase;
}

static void check_ring(const Arena& a, const Desc& d, const Tables& tb) {
  const int32_t nt = a.nt();
  const int64_t G = std::max<int32_t>(d.ring_grid, 1);
  const int64_t want_hold = d.ring_kind == 1 ? (d.ring_hold_override > 0 ? std::min(G, d.ring_hold_override) : G)
                                             : (d.ring_hold_override > 0 ? d.ring_hold_override : (int64_t)d.ring_slots * d.ring_grid);
  CHECK(tb.ring_hold_max == want_hold);
  CHECK((int32_t)tb.ring_t.size() == nt);
  std::vector<Ranges> quant(nt), publish(nt);
  std::vector<int64_t> last_norm(nt, -1), first_quant(nt, -1), first_hold(nt, -1), last_hold(nt, -1);
  for (size_t i = 0; i < tb.ring.size(); ++i) {
    const R::Item& it = tb.ring[i];
    if (it.begin == it.end) {  // an empty item keeps the register-resident rows aligned
      CHECK(d.ring_kind == 1 && it.flags == 0);
      continue;
    }
    CHECK(it.tensor >= 0 && it.tensor < nt);
    if (it.tensor < 0 || it.tensor >= nt) continue;
    const int32_t t = it.tensor;
    const R::Tensor& T = tb.ring_t[t];
    CHECK(it.flags == R::kPublish || it.flags == R::kQuant || it.flags == (R::kPublish | R::kQuant));
    CHECK(it.tbegin == a.offsets[t] && it.tn == a.sizes[t] && it.nchunks == T.nchunks && it.gbase == T.gbase);
    CHECK(it.chunk >= 0 && it.chunk < T.nchunks);
    CHECK(it.begin == it.tbegin + (int64_t)it.chunk * d.ring_chunk);
    CHECK(it.end == std::min(it.tbegin + it.tn, it.begin + d.ring_chunk));
    if (it.flags & R::kQuant) quant[t].emplace_back(it.begin, it.end);
    if (it.flags & R::kPublish) publish[t].emplace_back(it.begin, it.end);
    if (it.flags == R::kPublish) last_norm[t] = (int64_t)i;
    if (it.flags == R::kQuant && first_quant[t] < 0) first_quant[t] = (int64_t)i;
    if (it.flags == (R::kPublish | R::kQuant)) {
      if (first_hold[t] < 0) first_hold[t] = (int64_t)i;
      last_hold[t] = (int64_t)i;
    }
  }
  int64_t gbase = 0, two_pass = 0;
  for (int32_t t = 0; t < nt; ++t) {
    const int64_t b = a.offsets[t], n = a.sizes[t];
    const R::Tensor& T = tb.ring_t[t];
    CHECK(T.begin == b && T.n == n && T.nchunks == (n + d.ring_chunk - 1) / d.ring_chunk);
    CHECK(T.gbase == gbase);  // granules: disjoint, in order
    gbase += T.nchunks;
    CHECK(tiles(quant[t], b, b + n));
    CHECK(tiles(publish[t], b, b + n));
    const bool big = T.nchunks > tb.ring_hold_max;
    two_pass += big;
    CHECK(big == (last_norm[t] >= 0) && big == (first_quant[t] >= 0) && big == (first_hold[t] < 0));
    CHECK(!big || last_norm[t] < first_quant[t]);
    if (!big && d.ring_kind == 1) {  // a single-read tensor lies in one row of G items, chunks adjacent
      CHECK(first_hold[t] / G == last_hold[t] / G);
      CHECK(last_hold[t] - first_hold[t] + 1 == T.nchunks);
    }
  }
  if (d.ring_kind == 0 && d.ring_big_mode == 1) {  // every NORM chunk first, every QUANT chunk last
    int64_t norms = 0, quants = 0;
    for (const R::Item& it : tb.ring) {
      norms += it.flags == R::kPublish;
      quants += it.flags == R::kQuant;
    }
    for (int64_t i = 0; i < (int64_t)tb.ring.size(); ++i) {
      CHECK((tb.ring[i].flags == R::kPublish) == (i < norms));
      CHECK((tb.ring[i].flags == R::kQuant) == (i >= (int64_t)tb.ring.size() - quants));
    }
  }
  CHECK(tb.ring_two_pass == two_pass);
  CHECK(tb.n_ring_gran == std::max<int64_t>(gbase, 1));
}

static void check_flat(const Arena& a, const Tables& tb) {
  const int32_t nt = a.nt();
  constexpr int64_t kItemParts = kBlkWaves * (kSub / kSpecBlk);
  CHECK(tb.n_flat == (int64_t)tb.flat.size() && tb.n_spec_blocks == 4 * tb.n_flat);
  CHECK((int32_t)tb.br_items.size() == nt && (int32_t)tb.grid_pbeg.size() == nt && (int32_t)tb.grid_pcnt.size() == nt);
  std::vector<Ranges> cover(nt);
  for (size_t i = 0; i < tb.flat.size(); ++i) {
    const Item& it = tb.flat[i];
    CHECK(it.tensor >= 0 && it.tensor < nt && it.kind == kQuant);
    if (it.tensor < 0 || it.tensor >= nt) continue;
    CHECK(i == 0 || tb.flat[i - 1].tensor <= it.tensor);  // tensor order: a tensor's items are adjacent
    CHECK(it.begin == a.offsets[it.tensor] + (int64_t)it.chunk * kSub && it.end - it.begin <= kSub);
    cover[it.tensor].emplace_back(it.begin, it.end);
  }
  int64_t item = 0;
  int32_t sbase = 0;
  size_t f = 0;
  for (int32_t t = 0; t < nt; ++t) {
    const int64_t b = a.offsets[t], n = a.sizes[t];
    CHECK(tiles(cover[t], b, b + n));
    CHECK(tb.grid_pbeg[t] == (uint32_t)item && tb.grid_pcnt[t] == (uint32_t)cover[t].size());
    const SpecBrItem& br = tb.br_items[t];
    CHECK(br.tensor == t && br.begin == b && br.n == n);
    CHECK(br.R >= 1 && br.R <= kSpecRuns && (br.R == 1 || (int64_t)br.R * 2 * kSpecRun <= n));
    CHECK(br.base * br.R + br.rem == n && br.rem >= 0 && br.rem < br.R);
    CHECK(br.Rw >= 1 && br.Rw <= kSpecRunsWide && (br.Rw == 1 || (int64_t)br.Rw * 2 * kSpecRunWide <= n));
    // fold segments: the tensor's wave partials [p0, p1), in order, kSpecSeg each but the last
    const int64_t p0 = kItemParts * item, p1 = kItemParts * (item + (int64_t)cover[t].size());
    const int32_t nsegs = (int32_t)((p1 - p0 + kSpecSeg - 1) / kSpecSeg);
    int64_t at = p0;
    for (int32_t q = 0; q < nsegs; ++q, ++f) {
      CHECK(f < tb.fold_items.size());
      if (f >= tb.fold_items.size()) break;
      const SpecFoldItem& fi = tb.fold_items[f];
      CHECK(fi.tensor == t && fi.seg == q && fi.nsegs == nsegs && fi.sbase == sbase);
      CHECK(fi.p_begin == at && fi.p_end == std::min(p1, at + kSpecSeg));
      at = fi.p_end;
    }
    CHECK(at == p1);
    sbase += nsegs;
    item += (int64_t)cover[t].size();
  }
  CHECK(f == tb.fold_items.size() && item == tb.n_flat);
}

static void check_dec_blocks(const Arena& a, const Tables& tb) {
  CHECK((int64_t)tb.dec_binfo.size() == (a.end() + kDecBlk - 1) / kDecBlk);
  for (size_t k = 0; k < tb.dec_binfo.size(); ++k) {
    const int64_t base = (int64_t)k * kDecBlk;
    int32_t t = a.nt() - 1;
    while (t > 0 && a.offsets[t] > base) --t;  // the last tensor starting at or before the block
    const bool inside = a.offsets[t] <= base && base + kDecBlk <= a.offsets[t] + a.sizes[t];
    CHECK((tb.dec_binfo[k] & 0x7fffffffu) == (uint32_t)t);
    CHECK((tb.dec_binfo[k] >> 31) == (inside ? 1u : 0u));
  }
}

struct RingCfg {
  int64_t chunk;
  int32_t slots, kind;
};
// omf_qsgd_ring.hip kConfigs: the LDS rings of 64 KiB x 2 and 32 KiB x 4 slots, the register-resident ones
static const RingCfg kRing[] = {{16384, 2, 0}, {8192, 4, 0}, {16384, 4, 1}, {16384, 3, 1}};

static void check_tables(const Arena& a, Desc d, const char* name) {
  d.sizes = a.sizes.data();
  d.offsets = a.offsets.data();
  d.nt = a.nt();
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s ev=%d cap=%lld ring=%lld/%d/%d grid=%d big=%d gap=%lld hold=%lld", name, d.ev,
                (long long)d.cap, (long long)d.ring_chunk, d.ring_slots, d.ring_kind, d.ring_grid, d.ring_big_mode,
                (long long)d.ring_gap, (long long)d.ring_hold_override);
  g_case = buf;
  Tables tb;
  CHECK(build_tables(d, tb));
  CHECK(tb.n_enc[0] == (int64_t)tb.enc[0].size() && tb.n_enc[1] == (int64_t)tb.enc[1].size());
  const int64_t np0 = check_enc(a, d, tb.enc[0], tb.tinfo[0], true);
  const int64_t np1 = check_enc(a, d, tb.enc[1], tb.tinfo[1], false);
  CHECK(tb.n_partials == std::max<int64_t>(std::max(np0, np1), 1));
  check_ring(a, d, tb);
  check_flat(a, tb);
  check_dec_blocks(a, tb);
}

static void sweep(const Arena& a, Desc base, const char* name) {
  for (const RingCfg& rc : kRing)
    for (int big = 0; big <= 1; ++big)
      for (int64_t gap : {(int64_t)-1, (int64_t)0, (int64_t)3})
        for (int ev : {8, 16}) {
          Desc d = base;
          d.ring_chunk = rc.chunk;
          d.ring_slots = rc.slots;
          d.ring_kind = rc.kind;
          d.ring_big_mode = big;
          d.ring_gap = gap;
          d.ev = ev;
          check_tables(a, d, name);
        }
}

static void check_all_tables() {
  Desc d;  // chunk 2 x 16 Ki, one resident item, a grid of 4
  d.ring_grid = 4;
  d.cap = 4;
  sweep(Arena({1}), d, "one element");
  sweep(Arena({1, 3, 4, 5}), d, "1 3 4 5");
  sweep(Arena({16384, 16385}), d, "16384 16385");
  sweep(Arena({8197, 16385, 70001, 1 << 20}), d, "four tensors");
  for (const RingCfg& rc : kRing) {  // one ring chunk more than is held, between two small tensors
    Desc h = d;
    h.ring_hold_override = 2;
    sweep(Arena({5, 3 * rc.chunk, 100, 3 * rc.chunk - 1, 2 * rc.chunk}), h, "hold_max + 1 chunks");
  }
  // more than one fold segment (over kSpecSeg wave partials: 4 Mi elements), then a second tensor's
  sweep(Arena({(4 << 20) + 1, 100, 70001}), d, "4 Mi + 1");
  for (const RingCfg& rc : kRing)  // several packed rows with room left and no NORM item to fill it
    sweep(Arena({3 * rc.chunk, 3 * rc.chunk - 5, 2 * rc.chunk + 1, 2 * rc.chunk, 5}), d, "rows of 3 3 3 2 1 chunks");
  for (int64_t cap : {1, 2}) {  // 2 x chunk + 1 elements: resident only if its items fit the capacity
    Desc c = d;
    c.cap = cap;
    sweep(Arena({2 * c.chunk + 1}), c, "2 chunk + 1");
    sweep(Arena({7, 2 * c.chunk + 1, 16 * 1024 + 1}), c, "7, 2 chunk + 1, 16 Ki + 1");
  }
}

static void check_carve() {
  g_case = "carve";
  uint8_t* a = nullptr;
  uint32_t* b = nullptr;
  double* c = nullptr;
  Item* d = nullptr;
  uint64_t* e = nullptr;
  uint32_t* f = nullptr;
  const std::vector<uint32_t> hb = {1, 2, 3, 4, 5};
  const std::vector<Item> hd(3);
  Carve cv;
  cv.zero(a, 33);
  cv.copy(b, hb);
  cv.raw(c, 1);
  cv.copy(d, hd);
  cv.zero(e, 0);  // an empty region takes no bytes
  cv.raw(f, 7);
  const std::vector<Carve::Region>& r = cv.regions();
  CHECK(r.size() == 6);
  const size_t want_bytes[6] = {33, 20, 8, 3 * sizeof(Item), 0, 28};
  size_t at = 0;
  for (size_t i = 0; i < r.size(); ++i) {
    CHECK(r[i].offset % 16 == 0);
    CHECK(r[i].offset >= at);               // declaration order, no overlap
    CHECK(r[i].offset - at < 16);           // and no more than the rounding between regions
    CHECK(r[i].bytes == want_bytes[i]);
    at = r[i].offset + r[i].bytes;
  }
  CHECK(r[0].offset == 0 && r[0].zero && !r[0].src);
  CHECK(r[1].src == hb.data() && !r[1].zero && r[3].src == hd.data());
  CHECK(!r[2].src && !r[2].zero);
  CHECK(cv.bytes() % 16 == 0 && cv.bytes() >= at && cv.bytes() - at < 16);
  std::vector<unsigned char> block(cv.bytes() + 16);
  unsigned char* base = block.data() + (16 - (uintptr_t)block.data() % 16) % 16;
  cv.bind(base);
  CHECK((unsigned char*)a == base && (unsigned char*)b == base + r[1].offset && (unsigned char*)c == base + r[2].offset);
  CHECK((unsigned char*)d == base + r[3].offset && (unsigned char*)f == base + r[5].offset);
  b[4] = 9u;  // the last element of a region is inside the allocation (the sanitizer checks the store)
  f[6] = 9u;
  cv.bind(nullptr);
  CHECK(!a && !b && !c && !d && !e && !f);
}

// ---------------------------------------------------------------- the encoder choice
static const int kBitsSwept[] = {0, 1, 4, 5, 6, 7, 8, 9};

// Rows "strategy bits caller_u caller_norms fmt divide last_client wide_levels fused_bracket grid_fits op encoder":
// the choice of that call equals (op '=') or differs from (op '!') `encoder`, or it or the call without divide
// and last client chooses it (op '|').
static int check_choice_rows(const char* path) {
  g_case = "choice rows";
  std::FILE* fh = std::fopen(path, "r");
  if (!fh) {
    std::printf("cannot open %s\n", path);
    return -1;
  }
  int rows = 0, st, s, u, ni, fmt, div, last, wl, fb, fits, enc;
  char op;
  while (std::fscanf(fh, "%d %d %d %d %d %d %d %d %d %d %c %d", &st, &s, &u, &ni, &fmt, &div, &last, &wl, &fb, &fits, &op,
                     &enc) == 12) {
    Call c;
    c.strategy = st;
    c.bits = s;
    c.caller_u = u != 0;
    c.caller_norms = ni != 0;
    c.fmt = (uint32_t)fmt;
    c.divide = div != 0;
    c.last_client = last != 0;
    c.wide_levels = wl != 0;
    c.fused_bracket = fb != 0;
    c.grid_fits = fits != 0;
    const Choice ch = choose_encoder(c);
    Call plain = c;
    plain.divide = plain.last_client = false;
    const bool ok = op == '='   ? ch.encoder == enc
                    : op == '!' ? ch.encoder != enc
                                : ch.encoder == enc || choose_encoder(plain).encoder == enc;
    if (!ok && ++g_fail <= 20)
      std::printf("FAIL choice row %d: %d %d %d %d %d %d %d %d %d %d %c %d, chose %d\n", rows, st, s, u, ni, fmt, div, last,
                  wl, fb, fits, op, enc, (int)ch.encoder);
    ++rows;
  }
  std::fclose(fh);
  return rows;
}

// The whole input space: what must hold of every choice, and how the inputs the recorded rows do
// not reach (debug bit 0, a switch under a strategy that ignores it, norms only) relate to those they do.
static void check_choice_space() {
  g_case = "choice space";
  for (int st = 0; st <= 4; ++st)
    for (int s : kBitsSwept)
      for (int bitsmask = 0; bitsmask < (1 << 8); ++bitsmask)
        for (uint32_t fmt = 0; fmt <= 2; ++fmt) {
          Call c;
          c.strategy = st;
          c.bits = s;
          c.fmt = fmt;
          c.caller_u = bitsmask & 1;
          c.caller_norms = (bitsmask >> 1) & 1;
          c.divide = (bitsmask >> 2) & 1;
          c.last_client = (bitsmask >> 3) & 1;
          c.wide_levels = (bitsmask >> 4) & 1;
          c.fused_bracket = (bitsmask >> 5) & 1;
          c.spec_dbg = (bitsmask >> 6) & 1;
          c.grid_fits = (bitsmask >> 7) & 1;
          const Choice ch = choose_encoder(c);
          CHECK(ch.encoder >= kEncResident && ch.encoder <= kEncCallerNorms);
          if (ch.encoder != kEncBracket) {
            CHECK(!ch.wide && !ch.fused && !ch.bracket_launch);
          } else {  // the variant: what the bracket launcher's tables are indexed by
            CHECK(st == 3 && !c.caller_u && !c.caller_norms && s >= 1 && s <= 8);
            CHECK(ch.wide == (s > 4));
            CHECK(!ch.wide || (c.wide_levels && fmt == 0 && !c.last_client));
            CHECK(fmt == 0 || !c.divide);
            CHECK(!(ch.fused && ch.bracket_launch));
            CHECK(ch.fused == (c.fused_bracket && fmt == 0 && !c.last_client && !c.spec_dbg));
            CHECK(ch.bracket_launch == (!ch.fused && !c.spec_dbg));  // bit 0 alone leaves the bracket out
          }
          CHECK((ch.encoder == kEncCallerNorms) == c.caller_norms);
          CHECK(ch.encoder != kEncGrid || (st == 4 && c.grid_fits && !c.caller_u && !c.divide));
          Call o = c;  // debug bit 0 never moves a call to another encoder
          o.spec_dbg ^= 1u;
          CHECK(choose_encoder(o).encoder == ch.encoder);
          if (st != 3) {  // the bracket's switches matter to strategy 3 alone
            o = c;
            o.wide_levels = !c.wide_levels;
            o.fused_bracket = !c.fused_bracket;
            CHECK(choose_encoder(o).encoder == ch.encoder);
          }
          if (st != 4) {
            o = c;
            o.grid_fits = !c.grid_fits;
            CHECK(choose_encoder(o).encoder == ch.encoder);
          }
          o = c;  // a norms-only pass: the ticket-ordered launch, whatever else is set
          o.norms_only = true;
          CHECK(choose_encoder(o).encoder == (st == 0 ? kEncResident : kEncOrdered));
        }
}

int main(int argc, char** argv) {
  check_all_tables();
  check_carve();
  int rows = 0;
  if (argc > 1) {
    rows = check_choice_rows(argv[1]);
    if (rows <= 0) {
      std::printf("no choice rows read from %s\n", argv[1]);
      return 2;
    }
  }
  check_choice_space();
  std::printf("plan_layout_check: %d failures, %d choice rows\n", g_fail, rows);
  return g_fail ? 1 : 0;
}
