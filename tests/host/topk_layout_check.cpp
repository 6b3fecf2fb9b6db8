// topk_layout_check.cpp — stand-alone CPU checker of omnifed_amd/csrc/omf_topk_layout.{h,cpp}
// (tests/test_topk_layout_host.py builds it with the sanitizers and runs it).
//
//   topk_layout_check arenas.txt
//
// One arena per line of the file: name ratio tmp_bytes expected_total(-1: none) nt size offset ...
// (the test writes the plans of tests/golden/topk_matrix_inputs.py).  Those and a set of tiny arenas
// of its own are run at sample sizes 64 / 2048 / 2^20 and group counts 1 / 2 / 3 / 16 / nt + 3: the
// encode tables, the groups, the encode workspace, the decode tables and workspace are held to what
// the kernels rely on, and the flat-item ranges to plan_layout::build_tables.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../omnifed_amd/csrc/omf_plan_layout.h"
#include "../../omnifed_amd/csrc/omf_topk_layout.h"

using namespace omf::topk_layout;
namespace PL = omf::plan_layout;

static int g_fail = 0, g_cases = 0;
static std::string g_case;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (++g_fail <= 20) std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond); \
    }                                                                                    \
  } while (0)

struct Arena {
  std::string name;
  std::vector<int64_t> sizes, offsets;
  double ratio = 0.01;
  size_t tmp_bytes = 4 * 256 * 256;
  int64_t expect_total = -1;
  int32_t nt() const { return (int32_t)sizes.size(); }
  int64_t end() const { return offsets.back() + sizes.back(); }
};

static Arena tiny(const char* name, std::vector<int64_t> sizes, double ratio) {
  Arena a;
  a.name = name;
  a.sizes = std::move(sizes);
  a.ratio = ratio;
  int64_t o = 0;
  for (int64_t n : a.sizes) {  // codec.arena_layout: tensors start on multiples of 64 elements
    a.offsets.push_back(o);
    o = (o + n + 63) / 64 * 64;
  }
  return a;
}

template <class V>
static bool is_prefix(const V& pre, size_t nt, auto per_tensor) {  // exclusive prefix sums, the total at nt
  if (pre.size() != nt + 1 || pre[0] != 0) return false;
  for (size_t t = 0; t < nt; ++t)
    if (pre[t + 1] - pre[t] != per_tensor(t)) return false;
  return true;
}

// ---------------------------------------------------------------- encode tables
static void check_tables(const Arena& a, const EncodeTables& tb, int64_t max_runs) {
  const size_t nt = a.sizes.size();
  CHECK(tb.kk.size() == nt && tb.kb2.size() == nt && tb.tfirst.size() == nt && tb.tlast.size() == nt);
  if (tb.kk.size() != nt || tb.kb2.size() != nt || tb.tfirst.size() != nt || tb.tlast.size() != nt) return;
  for (size_t t = 0; t < nt; ++t) CHECK(tb.kk[t] == topk_k(a.sizes[t], a.ratio) && tb.kk[t] >= 1);
  CHECK(is_prefix(tb.koff, nt, [&](size_t t) { return topk_k(a.sizes[t], a.ratio); }));
  CHECK(is_prefix(tb.bbase, nt, [&](size_t t) { return bucket_slots(topk_k(a.sizes[t], a.ratio)); }));
  CHECK(is_prefix(tb.sbase, nt, [&](size_t t) { return tensor_supers(tensor_items(a.sizes[t])); }));
  if (tb.koff.size() != nt + 1 || tb.sbase.size() != nt + 1 || tb.bbase.size() != nt + 1) return;
  for (size_t t = 0; t < nt; ++t) CHECK(tb.kb2[t] == tb.koff[t] + (int64_t)t * kBucketPad);
  // the flat items of the plan's own tables
  PL::Desc d;
  d.sizes = a.sizes.data();
  d.offsets = a.offsets.data();
  d.nt = a.nt();
  PL::Tables pt;
  CHECK(PL::build_tables(d, pt));
  for (size_t t = 0; t < nt; ++t) {
    int64_t first = -1, last = -1, count = 0;
    for (size_t i = 0; i < pt.flat.size(); ++i)
      if (pt.flat[i].tensor == (int32_t)t) {
        if (first < 0) first = (int64_t)i;
        last = (int64_t)i;
        ++count;
      }
    CHECK(first == (int64_t)tb.tfirst[t] && last == (int64_t)tb.tlast[t] && count == last - first + 1);
    CHECK(count == tensor_items(a.sizes[t]));
  }
  // super-items: runs of at most kSupItems items tiling each tensor's items, the flag once per tensor
  CHECK(tb.supinfo.size() == 4 * (size_t)tb.sbase[nt]);
  {
    size_t s = 0;
    for (size_t t = 0; t < nt && tb.supinfo.size() == 4 * (size_t)tb.sbase[nt]; ++t) {
      CHECK(s == tb.sbase[t]);
      uint32_t at = tb.tfirst[t];
      int flags = 0;
      for (; s < tb.sbase[t + 1]; ++s) {
        const uint32_t* e = &tb.supinfo[4 * s];
        CHECK(e[0] == t && e[1] == at && e[2] >= 1 && e[2] <= (uint32_t)kSupItems);
        CHECK(e[3] == (at == tb.tfirst[t] ? 1u : 0u));
        flags += (int)e[3];
        at += e[2];
      }
      CHECK(at == tb.tlast[t] + 1 && flags == 1);
    }
  }
  // sample blocks: each tensor's runs [0, ceil(n / stride)) in steps of kSRunsPerBlock
  {
    size_t b = 0;
    for (size_t t = 0; t < nt; ++t) {
      const int64_t n = a.sizes[t];
      const int64_t stride = std::max<int64_t>(kSStride, (n + max_runs - 1) / max_runs);  // the rule, spelled out
      CHECK(stride == sample_stride(n, max_runs));
      const int64_t nr = (n + stride - 1) / stride;
      CHECK(nr >= 1 && nr <= max_runs && nr == sample_runs(n, stride));
      CHECK(tb.sblk[t] == b);
      for (int64_t r0 = 0; r0 < nr; r0 += kSRunsPerBlock, ++b) {
        CHECK(2 * b + 1 < tb.smap.size());
        if (2 * b + 1 >= tb.smap.size()) return;
        CHECK(tb.smap[2 * b] == t && tb.smap[2 * b + 1] == (uint32_t)r0);
      }
      CHECK(b - tb.sblk[t] == sample_blocks(nr));
    }
    CHECK(tb.smap.size() == 2 * b && tb.nsb == (int32_t)b && tb.sblk[nt] == b);
  }
  // zero-fill chunks: [0, k_t) of each tensor exactly once in kZChunk steps
  {
    size_t c = 0;
    for (size_t t = 0; t < nt; ++t)
      for (int64_t x = 0; x * kZChunk < tb.kk[t]; ++x, ++c) {
        CHECK(2 * c + 1 < tb.zmap.size());
        if (2 * c + 1 >= tb.zmap.size()) return;
        CHECK(tb.zmap[2 * c] == t && tb.zmap[2 * c + 1] == (uint32_t)x);
      }
    CHECK(tb.zmap.size() == 2 * c && tb.nzb == (int32_t)c);
  }
  // the device table: 256-byte aligned disjoint regions that hold the vectors, the zeroed tail
  const SetupCarve sc = setup_table_carve(tb);
  size_t at = 0;
  const std::map<std::string, size_t> need = {
      {"kk", 8 * nt}, {"koff", 8 * (nt + 1)}, {"kb2", 8 * nt}, {"tfirst", 4 * nt}, {"tlast", 4 * nt},
      {"bbase", 4 * (nt + 1)}, {"sbase", 4 * (nt + 1)}, {"smap", 4 * tb.smap.size()},
      {"supinfo", 4 * tb.supinfo.size()}, {"zmap", 4 * tb.zmap.size()}, {"done", 16}, {"arrive", 4 * nt},
      {"gz", 4 * nt}, {"gh", 4 * nt * (size_t)kSBins}};
  CHECK(sc.carve.regions().size() == need.size());
  for (const auto& r : sc.carve.regions()) {
    CHECK(r.offset % 256 == 0 && r.offset >= at);
    CHECK(need.count(r.name) && r.bytes >= need.at(r.name));
    if (!std::strcmp(r.name, "done")) CHECK(r.offset == sc.zero_begin);
    at = r.offset + r.bytes;
  }
  CHECK(at <= sc.carve.bytes());
}

// ---------------------------------------------------------------- groups
static void check_groups(const Arena& a, const EncodeTables& tb, int64_t max_runs, int G) {
  const int32_t nt = a.nt();
  const std::vector<Group> gs = make_groups(tb, G);
  CHECK(!gs.empty() && (int)gs.size() <= std::max(1, std::min(G, (int)nt)));
  if (G == 1) CHECK(gs.size() == 1);
  int32_t t = 0;
  uint32_t sb = 0, sub = 0, sup = 0, bk = 0;
  for (const Group& g : gs) {
    CHECK(g.t0 == t && g.t1 > g.t0 && g.t1 <= nt);
    CHECK(g.sb0 == sb && g.sub0 == sub && g.sup0 == sup && g.bk0 == bk);
    uint32_t nsb = 0, nsub = 0, nsup = 0, nbk = 0, nb_max = 0;
    for (int32_t u = g.t0; u < g.t1 && u < nt; ++u) {
      const int64_t n = a.sizes[(size_t)u];
      nsb += sample_blocks(sample_runs(n, sample_stride(n, max_runs)));
      nsub += (uint32_t)(tensor_items(n) * kSubsPerItem);
      nsup += tensor_supers(tensor_items(n));
      const uint32_t nb = bucket_slots(topk_k(n, a.ratio));
      nbk += nb;
      nb_max = std::max(nb_max, nb);
    }
    CHECK(g.nsb == nsb && g.nsub == nsub && g.nsup == nsup && g.nbk == nbk && g.nb_max == nb_max);
    sb += nsb, sub += nsub, sup += nsup, bk += nbk;
    t = g.t1;
  }
  CHECK(t == nt);
  CHECK(sb == (uint32_t)tb.nsb && sup == tb.sbase[(size_t)nt] && bk == tb.bbase[(size_t)nt]);
  CHECK(sub == (tb.tlast[(size_t)nt - 1] + 1) * (uint32_t)kSubsPerItem);
}

// ---------------------------------------------------------------- encode workspace
template <class S>
static void check_carve(const Carve<S>& c) {  // aligned, in order, disjoint, inside, total = sum of aligned sizes
  size_t at = 0, sum = 0;
  for (const auto& r : c.regions()) {
    CHECK(r.offset % 256 == 0);
    CHECK(r.offset >= at);
    at = r.offset + r.bytes;
    sum += align256(r.bytes);
  }
  CHECK(at <= c.bytes());
  CHECK(sum == c.bytes());
}

static EncodeWsLayout check_ws(const Arena& a) {
  const EncodeWsLayout L = encode_ws_layout(a.sizes, a.end(), a.tmp_bytes);
  const size_t nt = a.sizes.size(), ae = (size_t)a.end();
  size_t items = 0, slots = 0;
  for (int64_t n : a.sizes) {
    items += (size_t)((n + kSub - 1) / kSub);
    slots += 2 * (size_t)(n / kBucketHalf) + 3;  // bucket_slots at k = n: the most any ratio needs
  }
  CHECK(L.nb_max == slots);
  // what the kernels index, per region (bytes)
  const std::map<std::string, size_t> need = {
      {"hist", 4 * nt * (size_t)kBins}, {"bin", 4 * nt}, {"cnt", 4 * nt}, {"flag", 4 * nt},
      {"status", 4 * 9},  // the verdict words [0, 3], the exact tail's [4, 8]
      {"tkey", 4 * nt}, {"zcnt", 4 * nt}, {"seg_b", 4 * nt}, {"seg_e", 4 * nt}, {"cstart", 8 * nt},
      {"sub_cnt", 4 * items * (size_t)kSubsPerItem}, {"item_cnt", 4 * items}, {"item_off", 4 * items},
      {"cand", 8 * ae}, {"sorted", 8 * (ae + nt * (size_t)kBucketPad)}, {"fmap", 4 * nt * (size_t)kCoarse},
      {"tlo", 4 * nt}, {"thi", 4 * nt}, {"fcount", 4 * nt}, {"fhist", 4 * nt * (size_t)kFineMax},
      {"fbucket", 4 * nt * (size_t)kFineMax}, {"bstart", 4 * slots},
      {"brec", sizeof(BucketRec) * slots}, {"bfill", 4 * slots}, {"tmp", a.tmp_bytes}};
  CHECK(L.carve.regions().size() == need.size());
  check_carve(L.carve);
  CHECK(L.total == L.carve.bytes() && L.tmp_bytes == a.tmp_bytes);
  std::vector<std::string> zeroed;
  for (const auto& r : L.carve.regions()) {
    CHECK(need.count(r.name) == 1);
    if (need.count(r.name)) CHECK(r.bytes >= need.at(r.name));
    if (r.offset < L.zero_end) {
      CHECK(r.offset + r.bytes <= L.zero_end);
      zeroed.push_back(r.name);
    }
  }
  CHECK((zeroed == std::vector<std::string>{"hist", "bin", "cnt", "flag", "status"}));
  // bind: every pointer at its region
  const std::unique_ptr<unsigned char[]> base(new unsigned char[L.total]);  // (never touched)
  const EncodeWs w = L.carve.bind(base.get());
  const auto& rg = L.carve.regions();
  CHECK((unsigned char*)w.hist == base.get() + rg.front().offset && w.tmp == base.get() + rg.back().offset);
  CHECK((unsigned char*)w.brec == base.get() + rg[rg.size() - 3].offset);
  if (a.expect_total >= 0) CHECK((int64_t)L.total == a.expect_total);
  return L;
}

// ---------------------------------------------------------------- decode
static void check_decode(const Arena& a, const std::vector<int64_t>& ks) {
  const size_t nt = a.sizes.size();
  const DecodeTables d = dec_tables_host(a.sizes, a.offsets, a.end(), ks.data());
  CHECK(is_prefix(d.koff, nt, [&](size_t t) { return ks[t]; }));
  CHECK(d.nsuper == (int32_t)((a.end() + 65535) / 65536) && d.nsuper == dec_nsuper(a.end()));
  CHECK(d.cap_base.size() == (size_t)d.nsuper + 1 && d.cap_base[0] == 0);
  if (d.koff.size() != nt + 1 || d.cap_base.size() != (size_t)d.nsuper + 1) return;
  for (int32_t q = 0; q < d.nsuper; ++q) {
    CHECK(d.cap_base[(size_t)q + 1] >= d.cap_base[(size_t)q]);
    const uint32_t step = d.cap_base[(size_t)q + 1] - d.cap_base[(size_t)q];
    CHECK(step >= 256 && step <= (1u << 16));
    // at least the selected values that can land in the super-tile when a tensor's k == n fills it
    int64_t full = 0;
    for (size_t t = 0; t < nt; ++t)
      if (ks[t] == a.sizes[t])
        full += std::max<int64_t>(0, std::min(a.offsets[t] + a.sizes[t], ((int64_t)q + 1) << 16) -
                                         std::max(a.offsets[t], (int64_t)q << 16));
    CHECK((int64_t)step >= std::min<int64_t>(full, 1 << 16));
  }
  const int64_t ktot = d.koff[nt], nb = dec_place_blocks(ktot);
  CHECK(nb == std::max<int64_t>(1, (ktot + kDecChunk - 1) / kDecChunk));
  CHECK(d.blk_t.size() == 2 * (size_t)nb);
  if (d.blk_t.size() != 2 * (size_t)nb) return;
  auto brute = [&](int64_t j) {  // the largest t with koff[t] <= j
    uint32_t best = 0;
    for (size_t t = 0; t < nt; ++t)
      if (d.koff[t] <= j) best = (uint32_t)t;
    return best;
  };
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t j0 = b * kDecChunk, j1 = std::max(std::min<int64_t>(j0 + kDecChunk, ktot), j0 + 1);
    CHECK(d.blk_t[2 * (size_t)b] == brute(j0));
    CHECK(d.blk_t[2 * (size_t)b + 1] == brute(j1 - 1));
    CHECK(d.blk_t[2 * (size_t)b + 1] < nt);
  }
  const Carve<DecWs> ws = dec_ws_layout(d.nsuper, d.cap_base.back(), ktot);
  check_carve(ws);
  CHECK(ws.regions().size() == 3);
  if (ws.regions().size() == 3) {
    CHECK(ws.regions()[0].bytes >= 4 * ((size_t)d.nsuper + 1));
    CHECK(ws.regions()[1].bytes >= 8 * (size_t)d.cap_base.back() && ws.regions()[1].bytes >= 8);
    CHECK(ws.regions()[2].bytes >= 8 * (size_t)std::max<int64_t>(ktot, 1));
  }
  const Carve<DecTable> tc = dec_table_carve((int32_t)nt, d.nsuper, nb);
  check_carve(tc);
  CHECK(tc.regions().size() == 3);
  if (tc.regions().size() == 3) {
    CHECK(tc.regions()[0].bytes >= 8 * d.koff.size() && tc.regions()[1].bytes >= 4 * d.cap_base.size());
    CHECK(tc.regions()[2].bytes >= 4 * d.blk_t.size());
  }
}

static void check_arena(Arena a) {
  CHECK(a.nt() >= 1);
  if (a.nt() < 1) return;
  for (int64_t max_runs : {(int64_t)64, (int64_t)2048, (int64_t)1 << 20}) {
    g_case = a.name + " ratio " + std::to_string(a.ratio) + " runs " + std::to_string(max_runs);
    const EncodeTables tb = build_encode_tables(a.sizes, a.ratio, max_runs);
    check_tables(a, tb, max_runs);
    for (int G : {1, 2, 3, 16, a.nt() + 3}) check_groups(a, tb, max_runs, G);
    ++g_cases;
  }
  g_case = a.name + " workspace";
  check_ws(a);
  g_case = a.name + " decode";
  std::vector<int64_t> ks;
  for (int64_t n : a.sizes) ks.push_back(topk_k(n, a.ratio));
  check_decode(a, ks);
  // zero counts at the start, in the middle and at the end; a k == n entry; nothing selected at all
  std::vector<int64_t> mixed = ks;
  for (size_t t = 0; t < mixed.size(); t += 3) mixed[t] = 0;
  mixed.back() = 0;
  if (mixed.size() > 1) mixed[1] = a.sizes[1];
  check_decode(a, mixed);
  std::reverse(mixed.begin(), mixed.end());
  for (size_t t = 0; t < mixed.size(); ++t) mixed[t] = std::min(mixed[t], a.sizes[t]);
  check_decode(a, mixed);
  check_decode(a, std::vector<int64_t>(a.sizes.size(), 0));
  check_decode(a, a.sizes);
}

int main(int argc, char** argv) {
  int from_file = 0;
  if (argc > 1) {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      Arena a;
      long long tmp = 0, expect = -1;
      int nt = 0;
      if (!(ls >> a.name >> a.ratio >> tmp >> expect >> nt)) continue;
      a.tmp_bytes = (size_t)tmp;
      a.expect_total = expect;
      for (int t = 0; t < nt; ++t) {
        long long n = 0, o = 0;
        ls >> n >> o;
        a.sizes.push_back(n);
        a.offsets.push_back(o);
      }
      g_case = a.name;
      CHECK(!ls.fail());
      if (ls.fail()) continue;
      check_arena(a);
      ++from_file;
    }
  }
  check_arena(tiny("one", {1}, 0.01));
  check_arena(tiny("one-full", {1}, 1.0));
  check_arena(tiny("sub-chunk", {511, 512, 513}, 0.3));
  check_arena(tiny("item", {16383, 16384, 16385}, 0.01));
  check_arena(tiny("item-full", {16383, 16384, 16385, 7}, 1.0));
  check_arena(tiny("two-supers", {32 * 16384 + 5, 100, 32 * 16384, 64 * 16384 + 1}, 0.05));
  check_arena(tiny("sampled-big", {5000000, 3, 300000}, 0.1));
  {
    std::vector<int64_t> s;  // more tensors than one 256-thread stripe
    for (int t = 0; t < 257; ++t) s.push_back(1 + (t * 977) % 20000);
    check_arena(tiny("nt257", s, 0.05));
  }
  // Two arenas of equal nt and arena_end and different sizes have different layouts: the bucket tables
  // are sized by the sum of bucket_slots(n_t) (152 against 40 slots here), not by nt and arena_end.
  {
    g_case = "pair";
    Arena a, b;
    a.name = "pair-a", b.name = "pair-b";
    for (int t = 0; t < 8; ++t) {
      a.offsets.push_back(16448 * t);
      b.offsets.push_back(16448 * t);
      a.sizes.push_back(16385);
      b.sizes.push_back(t == 7 ? 16385 : 513);
    }
    a.ratio = b.ratio = 0.05;
    CHECK(a.end() == b.end() && a.nt() == b.nt());
    const EncodeWsLayout la = check_ws(a), lb = check_ws(b);
    CHECK(la.nb_max == 152 && lb.nb_max == 40);
    CHECK(la.total != lb.total);
    auto bytes_of = [](const EncodeWsLayout& L, const char* name) {
      for (const auto& r : L.carve.regions())
        if (!std::strcmp(r.name, name)) return align256(r.bytes);
      return (size_t)0;
    };
    for (const char* name : {"bstart", "brec", "bfill"}) CHECK(bytes_of(la, name) > bytes_of(lb, name));
    check_arena(a);
    check_arena(b);
  }
  std::printf("%d failures, %d arenas from the file, %d cases\n", g_fail, from_file, g_cases);
  return g_fail ? 1 : 0;
}
