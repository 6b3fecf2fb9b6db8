// topk_pack_check.cpp — the host side of the bit-packed Top-K index wire on a CPU, under AddressSanitizer
// and UBSan: index_bits, pack_group / unpack_group (the routines the kernels of omf_topk_pack.hip call) and
// pack_tables_host (omf_topk_layout.{h,cpp}), against vectors tests/golden/topk_packed_inputs.py wrote.
//
// Records of the vector file (whitespace-separated integers after the tag):
//   B n b                                     index_bits(n) == b (b = -1: outside the range)
//   A nt (n_t k_t) x nt  bits x nt  goff x (nt + 1)  woff x (nt + 1)  words  idx x K  sent x words  dirty x words
//     the layout of the count vector; then the arena walked group by group as the kernels walk it: packing
//     idx gives `sent` word for word (codes 0 after each tensor's k_t-th index), unpacking `dirty` (= sent
//     with every bit past a tensor's k_t b set) gives idx and writes nothing else.
// Every buffer is a heap vector of its exact size, so a read or write past a group's words or a tensor's
// indices is an ASan report.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../omnifed_amd/csrc/omf_topk_layout.h"

using namespace omf::topk_layout;

static int g_fail = 0;
static std::string g_case;
#define CHECK(c)                                                                    \
  do {                                                                              \
    if (!(c)) {                                                                     \
      ++g_fail;                                                                     \
      if (g_fail <= 40) std::printf("FAIL %s: %s (line %d)\n", g_case.c_str(), #c, __LINE__); \
    }                                                                               \
  } while (0)

template <class T>
static std::vector<T> read_n(std::istream& in, size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) {
    long long x = 0;
    in >> x;
    v[i] = (T)x;
  }
  return v;
}

// The largest t with goff[t] <= g among [0, nt - 1], as koff_tensor on the device.
static int group_tensor(const std::vector<int64_t>& goff, int nt, int64_t g) {
  int lo = 0, hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (goff[(size_t)mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

static void check_bits(std::istream& in) {
  long long n = 0, b = 0;
  in >> n >> b;
  g_case = "index_bits(" + std::to_string(n) + ")";
  CHECK(index_bits((int64_t)n) == (int32_t)b);
}

static int g_widths[33];

static void check_arena(std::istream& in, int id) {
  g_case = "arena " + std::to_string(id);
  size_t nt = 0;
  in >> nt;
  std::vector<int64_t> sizes(nt), ks(nt);
  for (size_t t = 0; t < nt; ++t) in >> sizes[t] >> ks[t];
  const std::vector<int32_t> bits = read_n<int32_t>(in, nt);
  const std::vector<int64_t> goff = read_n<int64_t>(in, nt + 1), woff = read_n<int64_t>(in, nt + 1);
  long long words = 0;
  in >> words;
  const PackTables p = pack_tables_host(sizes, ks.data());
  CHECK(p.bits == bits);
  CHECK(p.goff == goff);
  CHECK(p.woff == woff);
  CHECK(p.words == (int64_t)words);
  CHECK(p.koff.size() == nt + 1 && p.koff[0] == 0);
  for (size_t t = 0; t < nt; ++t) {
    CHECK(p.koff[t + 1] - p.koff[t] == ks[t]);
    CHECK(bits[t] == index_bits(sizes[t]));
    CHECK(goff[t + 1] - goff[t] == (ks[t] + 31) / 32);          // a partial last group is a whole group
    CHECK(woff[t + 1] - woff[t] == (goff[t + 1] - goff[t]) * bits[t]);  // a group: b words, on a word
  }
  const int64_t K = p.koff[nt], G = goff[nt];
  const std::vector<int64_t> idx = read_n<int64_t>(in, (size_t)K);
  const std::vector<uint32_t> sent = read_n<uint32_t>(in, (size_t)words), dirty = read_n<uint32_t>(in, (size_t)words);
  if (g_fail) return;
  std::vector<uint32_t> got((size_t)words, 0xC0DEFACEu);
  std::vector<int64_t> back((size_t)K, -77);
  for (int64_t g = 0; g < G; ++g) {
    const int t = group_tensor(goff, (int)nt, g);
    CHECK(goff[(size_t)t] <= g && g < goff[(size_t)t + 1]);  // never an empty tensor
    const int64_t j = g - goff[(size_t)t], k0 = p.koff[(size_t)t];
    const int nv = (int)std::min<int64_t>(32, ks[(size_t)t] - 32 * j);
    CHECK(nv >= 1 && nv <= 32);
    const int b = bits[(size_t)t];
    ++g_widths[b];
    // each group's buffers of their exact sizes: nv indices, b words
    const std::vector<int64_t> in_idx(idx.begin() + k0 + 32 * j, idx.begin() + k0 + 32 * j + nv);
    std::vector<uint32_t> w((size_t)b, 0xC0DEFACEu);
    pack_group(in_idx.data(), nv, b, w.data());
    for (int i = 0; i < b; ++i) got[(size_t)(woff[(size_t)t] + j * b + i)] = w[(size_t)i];
    // unpack reads only the words that hold a code: hand it exactly those
    const size_t need = ((size_t)nv * (size_t)b + 31) / 32;
    const std::vector<uint32_t> dw(dirty.begin() + woff[(size_t)t] + j * b, dirty.begin() + woff[(size_t)t] + j * b + (int64_t)need);
    std::vector<int64_t> out((size_t)nv, -77);
    unpack_group(dw.data(), nv, b, out.data());
    for (int i = 0; i < nv; ++i) back[(size_t)(k0 + 32 * j + i)] = out[(size_t)i];
    std::vector<uint32_t> out32((size_t)nv, 7u);  // the kernels' LDS tile holds the codes as 32-bit words
    unpack_group(dw.data(), nv, b, out32.data());
    for (int i = 0; i < nv; ++i) CHECK((int64_t)out32[(size_t)i] == out[(size_t)i]);
  }
  CHECK(got == sent);    // every word of the arena written, pad codes 0
  CHECK(back == idx);    // exact whatever lies past k_t b
  // the low b bits are the code: an index with bits above b set packs as its low bits
  if (K > 0 && nt > 0) {
    size_t t = 0;
    while (ks[t] == 0) ++t;
    const int b = bits[t];
    const int64_t wild = idx[(size_t)p.koff[t]] | (b < 63 ? (int64_t)1 << (b + 20) : 0);
    std::vector<uint32_t> w1((size_t)b), w2((size_t)b);
    pack_group(&idx[(size_t)p.koff[t]], 1, b, w1.data());
    pack_group(&wild, 1, b, w2.data());
    CHECK(w1 == w2);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: topk_pack_check <vectors>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string tag;
  int n_bits = 0, n_arenas = 0;
  while (in >> tag) {
    if (tag == "B") {
      check_bits(in);
      ++n_bits;
    } else if (tag == "A") {
      check_arena(in, n_arenas++);
    } else {
      std::printf("unknown record %s\n", tag.c_str());
      return 2;
    }
    if (!in) {
      std::printf("truncated record %s\n", tag.c_str());
      return 2;
    }
  }
  int widths = 0;
  for (int b = 1; b <= 32; ++b) widths += g_widths[b] > 0;
  std::printf("%d failures, %d index_bits records, %d arenas, %d widths\n", g_fail, n_bits, n_arenas, widths);
  return g_fail ? 1 : 0;
}
