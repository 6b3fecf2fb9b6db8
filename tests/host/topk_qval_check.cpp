// topk_qval_check.cpp — the host side of the quantised Top-K value wire on a CPU, under AddressSanitizer and
// UBSan: the value-word layout rule (value_code_bits, value_group_word, value_words) and the group pack /
// unpack at the code widths b = 3..10, as the kernels of omf_topk_qval.hip use them (omf_topk_layout.{h,cpp}),
// against vectors tests/golden/topk_qval_inputs.py wrote.
//
// Records of the vector file (whitespace-separated integers after the tag):
//   S s b                                     value_code_bits(s) == b (b = -1: outside 1..8)
//   V nt (n_t k_t) x nt  s  words  codes x K  sent x words  dirty x words
//     the value arena of the count vector at value_bits s, walked group by group as the kernels walk it:
//     group g of the selection (tensor t's j-th group is g = goff[t] + j) at word g b; packing the 32-bit
//     codes gives `sent` word for word (codes 0 after each tensor's k_t-th value), unpacking `dirty` (= sent
//     with every bit past a tensor's k_t b set) gives the codes and reads no word past the last code's.
// Every buffer is a heap vector of its exact size, so a read or write past a group's words is an ASan report.
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

static int g_widths[16];

static void check_bits(std::istream& in) {
  long long s = 0, b = 0;
  in >> s >> b;
  g_case = "value_code_bits(" + std::to_string(s) + ")";
  CHECK(value_code_bits((int32_t)s) == (int32_t)b);
}

static void check_arena(std::istream& in, int id) {
  g_case = "arena " + std::to_string(id);
  size_t nt = 0;
  in >> nt;
  std::vector<int64_t> sizes(nt), ks(nt);
  for (size_t t = 0; t < nt; ++t) in >> sizes[t] >> ks[t];
  long long s = 0, words = 0;
  in >> s >> words;
  const int b = value_code_bits((int32_t)s);
  CHECK(b == (int)s + 2);
  const PackTables p = pack_tables_host(sizes, ks.data());
  CHECK(value_words(p, b) == (int64_t)words);
  const int64_t K = p.koff[nt], G = p.goff[nt];
  CHECK(value_group_word(G, b) == (int64_t)words && value_group_word(0, b) == 0);
  const std::vector<uint32_t> codes = read_n<uint32_t>(in, (size_t)K);
  const std::vector<uint32_t> sent = read_n<uint32_t>(in, (size_t)words), dirty = read_n<uint32_t>(in, (size_t)words);
  if (g_fail) return;
  std::vector<uint32_t> got((size_t)words, 0xC0DEFACEu), back((size_t)K, 0xFFFFFFFFu);
  for (int64_t g = 0; g < G; ++g) {
    const int t = group_tensor(p.goff, (int)nt, g);
    CHECK(p.goff[(size_t)t] <= g && g < p.goff[(size_t)t + 1]);
    const int64_t j = g - p.goff[(size_t)t], k0 = p.koff[(size_t)t];
    const int nv = (int)std::min<int64_t>(32, ks[(size_t)t] - 32 * j);
    CHECK(nv >= 1 && nv <= 32);
    ++g_widths[b];
    const int64_t w0 = value_group_word(g, b);
    CHECK(w0 + b <= (int64_t)words);  // consecutive groups tile the arena: b words each
    const std::vector<uint32_t> in_codes(codes.begin() + k0 + 32 * j, codes.begin() + k0 + 32 * j + nv);
    std::vector<uint32_t> w((size_t)b, 0xC0DEFACEu);
    pack_group(in_codes.data(), nv, b, w.data());
    for (int i = 0; i < b; ++i) got[(size_t)(w0 + i)] = w[(size_t)i];
    const size_t need = ((size_t)nv * (size_t)b + 31) / 32;  // unpack reads only the words that hold a code
    const std::vector<uint32_t> dw(dirty.begin() + w0, dirty.begin() + w0 + (int64_t)need);
    std::vector<uint32_t> out((size_t)nv, 7u);
    unpack_group(dw.data(), nv, b, out.data());
    for (int i = 0; i < nv; ++i) back[(size_t)(k0 + 32 * j + i)] = out[(size_t)i];
  }
  CHECK(got == sent);
  CHECK(back == codes);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: topk_qval_check <vectors>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string tag;
  int n_bits = 0, n_arenas = 0;
  while (in >> tag) {
    if (tag == "S") {
      check_bits(in);
      ++n_bits;
    } else if (tag == "V") {
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
  for (int b = 3; b <= 10; ++b) widths += g_widths[b] > 0;
  std::printf("%d failures, %d bits records, %d arenas, %d widths\n", g_fail, n_bits, n_arenas, widths);
  return g_fail ? 1 : 0;
}
