// qsgd_dec_check.cpp — stand-alone CPU checker of the host rules of omnifed_amd/csrc/omf_qsgd_dec.h
// (tests/test_qsgd_dec_host.py builds it with the sanitizers and runs it): the chaining rule of the
// K-client sums, the levels scale and the overlap test.  No HIP header is needed.
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../omnifed_amd/csrc/omf_qsgd_dec.h"

using namespace omf;

static int g_fail = 0, g_checks = 0;
static std::string g_case;
#define CHECK(cond)                                                                                           \
  do {                                                                                                        \
    ++g_checks;                                                                                               \
    if (!(cond)) {                                                                                            \
      if (++g_fail <= 20) std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_case.c_str(), #cond);     \
    }                                                                                                         \
  } while (0)

// The groups of one call, walked as both sum entry points walk them.
static void check_chain(int32_t nclients, int32_t per, int32_t init, float divisor) {
  g_case = "K=" + std::to_string(nclients) + " per=" + std::to_string(per) + " init=" + std::to_string(init) +
           " div=" + std::to_string(divisor);
  int32_t next = 0, groups = 0;
  for (int32_t k0 = 0; k0 < nclients; k0 += per, ++groups) {
    const SumGroup g = sum_group(nclients, per, init, divisor, k0);
    const bool first = k0 == 0, last = k0 + g.n == nclients;
    CHECK(k0 == next);  // in order, each client once
    CHECK(g.n >= 1 && g.n <= per);
    CHECK(last || g.n == per);  // only the last group may be short: the loop's stride is `per`
    next = k0 + g.n;
    CHECK(g.fill == ((first && !init) ? 1 : 0));
    CHECK(g.init == ((first && !init) ? 0 : 1));
    CHECK(last ? g.divisor == divisor : g.divisor == 0.0f);
    CHECK(g.pad_div == divisor);
  }
  CHECK(next == nclients);
  CHECK(groups == (nclients + per - 1) / per);
}

static void check_levels(int32_t levels) {
  g_case = "levels=" + std::to_string(levels);
  const LevelScale lv(levels);
  const bool pow2 = __builtin_popcount((uint32_t)levels) == 1;
  CHECK(lv.levels == (float)levels);
  CHECK(lv.pow2 == pow2);
  CHECK((lv.inv_levels * lv.levels == 1.0f) == pow2);
  if (!pow2) CHECK(lv.inv_levels == 0.0f);
}

int main() {
  for (const int32_t per : {4, 8})
    for (const int32_t n : {1, per - 1, per, per + 1, 2 * per, 2 * per + 1, 3 * per + 1})
      for (const int32_t init : {0, 1})
        for (const float divisor : {0.0f, 3.0f}) check_chain(n, per, init, divisor);

  for (const int32_t levels : {1, 2, 3, 10, 16, 127, 128, 1000, 1 << 30, INT32_MAX - 1}) check_levels(levels);

  g_case = "overlaps";
  alignas(16) static unsigned char buf[64];
  CHECK(!overlaps(buf, 16, buf + 16, 16));  // adjacent
  CHECK(!overlaps(buf + 16, 16, buf, 16));
  CHECK(overlaps(buf, 17, buf + 16, 16));  // one shared byte
  CHECK(overlaps(buf + 16, 16, buf, 17));
  CHECK(overlaps(buf, 64, buf + 8, 1));  // contained
  CHECK(!overlaps(buf + 8, 0, buf, 64));  // zero length, inside the other range
  CHECK(!overlaps(buf, 64, buf + 8, 0));
  CHECK(!overlaps(buf, 0, buf, 0));
  g_case = "aligned";
  CHECK(aligned(buf, 16) && aligned(buf + 4, 4) && !aligned(buf + 4, 16) && !aligned(buf + 1, 4));

  std::printf("%d failures, %d checks\n", g_fail, g_checks);
  return g_fail ? 1 : 0;
}
