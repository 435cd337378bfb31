// Stand-alone host check of the morphology trace's host part (csrc/bflbm_morph.h under BFLBM_MORPH_HOST_ONLY, on top of
// the host part of csrc/bflbm_fieldsel.h: no HIP, no library).  Built and run by tests/test_morph_abi.py with
// -fsanitize=address,undefined.  It checks
//   1. the levels of accepted arguments;
//   2. every refusal of the arguments, one bad argument each, the message compared in full;
//   3. the launch shape: the tiles, the chunk of planes and the work items, and the bound on a workgroup's cells.
// The level array lives on the heap at its exact length, so a read past nlevels is the sanitizer's.
// Prints "OK <checks>" and returns 0, or every failure and 1.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bflbm.h"
#define BFLBM_NHYDRO_ 22

namespace {
std::string g_msg;
int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_msg = buf;
  return 1;
}
}  // namespace

#define BFLBM_FIELDSEL_HOST_ONLY
#include "bflbm_fieldsel.h"
#define BFLBM_MORPH_HOST_ONLY
#include "bflbm_morph.h"

typedef std::vector<double> Doubles;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static void expect_refusal(const char* want, int source, int var, int nlevels, const Doubles* levels, int side) {
  g_msg.clear();
  const int rc = morph_refuse_args("X", source, var, nlevels, levels ? levels->data() : nullptr, side);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // ---- 1. the levels ---------------------------------------------------------------------------------------------------
  {
    const Doubles three = {0.5, -0.0, 1e200};
    g_msg.clear();
    expect(morph_refuse_args("X", 0, 21, 3, three.data(), 1) == 0 && g_msg.empty(), "good arguments pass");
    const MorphLevels L = morph_levels(3, three.data(), 1);
    expect(L.n == 3 && L.side == 1 && L.t[0] == 0.5 && L.t[1] == 0.0 && std::signbit(L.t[1]) && L.t[2] == 1e200, "the levels, bit for bit");
    expect(L.t[3] == 0.0 && L.t[7] == 0.0, "the unused entries");
    const Doubles eight(8, 1.0);
    expect(morph_refuse_args("X", 1, 8, 8, eight.data(), 0) == 0 && morph_levels(8, eight.data(), 0).t[7] == 1.0, "8 levels of the last hydrovsbar component pass");
    const Doubles huge = {std::numeric_limits<double>::max(), -std::numeric_limits<double>::max(), std::numeric_limits<double>::denorm_min()};
    expect(morph_refuse_args("X", 0, 0, 3, huge.data(), 0) == 0, "the largest and the smallest finite levels pass");
  }

  // ---- 2. refusals: one bad argument each ------------------------------------------------------------------------------
  const Doubles good = {0.25, 0.75};
  expect_refusal("X: 1..8 levels (got 0)", 0, 0, 0, &good, 0);
  expect_refusal("X: 1..8 levels (got 9)", 0, 0, 9, &good, 0);
  expect_refusal("X: 1..8 levels (got -1)", 0, 0, -1, &good, 0);
  expect_refusal("X: null argument", 0, 0, 2, nullptr, 0);
  {
    const Doubles l_nan = {0.25, nan}, l_inf = {inf, 0.75}, l_minf = {0.25, -inf};
    expect_refusal("X: level 1 is not finite (got nan)", 0, 0, 2, &l_nan, 0);
    expect_refusal("X: level 0 is not finite (got inf)", 0, 0, 2, &l_inf, 0);
    expect_refusal("X: level 1 is not finite (got -inf)", 0, 0, 2, &l_minf, 0);
  }
  expect_refusal("X: side must be 0 (v >= level) or 1 (v < level) (got 2)", 0, 0, 2, &good, 2);
  expect_refusal("X: side must be 0 (v >= level) or 1 (v < level) (got -1)", 0, 0, 2, &good, -1);
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got 2)", 2, 0, 2, &good, 0);
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got -1)", -1, 0, 2, &good, 0);
  expect_refusal("X: variable index 22 outside hydrovs (0..21)", 0, 22, 2, &good, 0);
  expect_refusal("X: variable index -1 outside hydrovs (0..21)", 0, -1, 2, &good, 0);
  expect_refusal("X: variable index 9 outside hydrovsbar (0..8)", 1, 9, 2, &good, 0);

  // ---- 3. the launch shape ---------------------------------------------------------------------------------------------
  expect(morph_tiles(1) == 1 && morph_tiles(1024) == 1 && morph_tiles(1025) == 2, "tiles of 1024 plane sites");
  // small boxes: the chunk falls to 8 planes, and to nz below that
  expect(morph_chunk(63, 5, 1) == 5 && morph_chunk(63, 8, 1) == 8 && morph_chunk(63, 19, 1) == 8 && morph_chunks(19, 8) == 3, "small boxes");
  expect(morph_items(63, 5, 1) == 1 && morph_items(63, 19, 1) == 3 && morph_items(2100, 19, 3) == 9, "work items per replica");
  // 256^3: 64 tiles; 64 planes leave 256 items, 32 leave 512, 16 leave 1024
  expect(morph_chunk(65536, 256, 1) == 16 && morph_items(65536, 256, 1) == 1024, "256^3: 16 planes, 1024 work items");
  // 16 replicas of 64^3: 4 tiles x 16 = 64 per chunk layer; 8 planes leave 512 < 1024: the smallest chunk
  expect(morph_chunk(4096, 64, 16) == 8 && morph_items(4096, 64, 16) == 32, "16 x 64^3: 8 planes");
  // 1024^3: 1024 tiles: 64 planes leave 16384 items
  expect(morph_chunk(1LL << 20, 1024, 1) == 64 && morph_items(1LL << 20, 1024, 1) == 16384, "1024^3: 64 planes");
  expect(3LL * morph_limits::kTile * morph_limits::kMaxChunk == 196608, "the most a 32-bit counter of a workgroup can reach");

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
