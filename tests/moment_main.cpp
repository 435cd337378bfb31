// Stand-alone host check of the moment trace's host part (csrc/bflbm_moment.h under BFLBM_MOMENT_HOST_ONLY: no HIP, no
// library).  Built and run by tests/test_moment_abi.py with -fsanitize=address,undefined.  It checks
//   1. the layout of a sample: W and the place of every word, against values written out by hand and against a walk that
//      visits every word exactly once;
//   2. the tile counts and the slices of the tree;
//   3. what a box is refused for, the message compared in full;
//   4. the launch shape and the buffers of the boxes the GPU tests run and of the measured workloads.
// Prints "OK <checks>" and returns 0, or every failure and 1.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

namespace {
std::string g_msg;
int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_msg = buf;
  return 1;
}
}  // namespace

#define BFLBM_MOMENT_HOST_ONLY
#include "bflbm_moment.h"

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static void expect_refusal(const char* want, int nx, int ny, int nz, int nrep) {
  g_msg.clear();
  const int rc = moment_refuse_box("X", nx, ny, nz, nrep);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

int main() {
  using namespace moment_limits;
  // ---- 1. the layout -----------------------------------------------------------------------------------------------------
  expect(kModes == 19 && kWords == 95, "W = 95");
  expect(moment_word_sum(0, 0) == 0 && moment_word_sum(0, 18) == 18 && moment_word_sum(1, 0) == 19 && moment_word_sum(1, 18) == 37, "sum: words 0..37, i = 19 fluid + a");
  expect(moment_word_sq(0, 0) == 38 && moment_word_sq(0, 18) == 56 && moment_word_sq(1, 0) == 57 && moment_word_sq(1, 18) == 75, "sq: words 38..75");
  expect(moment_word_cross(0) == 76 && moment_word_cross(7) == 83 && moment_word_cross(18) == 94, "cross: words 76..94");
  {
    std::vector<int> seen(kWords, 0);                        // on the heap at its exact length: a word outside is the sanitizer's
    for (int fluid = 0; fluid < 2; ++fluid)
      for (int a = 0; a < kModes; ++a) { seen[moment_word_sum(fluid, a)] += 1; seen[moment_word_sq(fluid, a)] += 1; }
    for (int a = 0; a < kModes; ++a) seen[moment_word_cross(a)] += 1;
    bool once = true;
    for (int w = 0; w < kWords; ++w) once = once && seen[w] == 1;
    expect(once, "every word exactly once");
  }
  for (int a = 0; a < kModes; ++a)
    expect(moment_word_sq(0, a) - moment_word_sum(0, a) == 38 && moment_word_sq(1, a) - moment_word_sum(1, a) == 38 && moment_word_cross(a) == 76 + a,
           "a mode's square lies 38 words after its sum");

  // ---- 2. the tiles and the slices ---------------------------------------------------------------------------------------
  expect(kTile == 2048 && kPerThread == 8 && kSlice == 12 && kLdsBytes == 49152, "the limits");
  expect(moment_tiles(33 * 7) == 1 && moment_tiles(64 * 32) == 1 && moment_tiles(70 * 33) == 2 && moment_tiles(16 * 16) == 1 && moment_tiles(2049) == 2
             && moment_tiles(256 * 256) == 32 && moment_tiles(64 * 64) == 2 && moment_tiles(kMaxPlaneSites) == (1 << 20) - 2,
         "tiles of 2048 sites of a plane");
  expect(moment_slices() == 8 && (moment_slices() - 1) * kSlice < kWords && moment_slices() * kSlice >= kWords && kWords - 7 * kSlice == 11,
         "8 slices of 12 accumulators, the last of 11");

  // ---- 3. refusals -------------------------------------------------------------------------------------------------------
  g_msg.clear();
  expect(moment_refuse_box("X", 70, 33, 4, 1) == 0 && moment_refuse_box("X", 256, 256, 256, 1) == 0 && moment_refuse_box("X", 64, 64, 64, 16) == 0 && g_msg.empty(), "the boxes in use");
  expect(moment_refuse_box("X", 1, 1, 65535, 65535) == 0 && moment_refuse_box("X", 46339, 46339, 1, 1) == 0 && g_msg.empty(), "the limits themselves");
  expect_refusal("X: nz = 65536 exceeds the 65535 planes of one launch", 8, 8, 65536, 1);
  expect_refusal("X: nz = 65536 exceeds the 65535 planes of one launch", 65536, 65536, 65536, 70000);          // before everything else
  expect_refusal("X: a plane of 2147483648 sites exceeds the 2147479552 of a 32-bit site index", 65536, 32768, 1, 1);
  expect_refusal("X: a plane of 2147479553 sites exceeds the 2147479552 of a 32-bit site index", 2147479553, 1, 1, 70000);
  expect_refusal("X: 65536 replicas exceed the 65535 of one launch", 8, 8, 8, 65536);

  // ---- 4. the launch shape and the buffers -------------------------------------------------------------------------------
  expect(moment_plane_words(1) == 95u && moment_plane_words(2) == 190u && moment_plane_words(32) == 3040u, "95 x tiles partials per plane");
  expect(moment_stage_words(1, 5, 1) == 475u && moment_stage_words(1, 3, 1) == 285u && moment_stage_words(1, 4, 2) == 760u, "(33, 7, 5), (64, 32, 3), (70, 33, 4)");
  expect(moment_stage_words(3, 8, 1) == 2280u && moment_stage_words(5, 8, 1) == 3800u, "3 and 5 replicas of (16, 8, 8)");
  expect(moment_stage_words(1, 256, 32) == 778240u && moment_stage_words(16, 64, 2) == 194560u, "256^3 and 16 x 64^3");
  expect(moment_stage_words(65535, 65535, 1) == 95ull * 65535ull * 65535ull, "the stage buffer is counted in 64 bits");

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
