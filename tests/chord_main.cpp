// Stand-alone host check of the chord trace's host part (csrc/bflbm_chord.h under BFLBM_CHORD_HOST_ONLY, on top of the host
// parts of csrc/bflbm_fieldsel.h, bflbm_hist.h and bflbm_morph.h: no HIP, no library).  Built and run by
// tests/test_chord_abi.py with -fsanitize=address,undefined.  It checks
//   1. accepted arguments, W and the offsets of the axis blocks;
//   2. every refusal of the arguments, one bad argument each and in the header's order, the message compared in full;
//   3. the counter cap at its edge;
//   4. the launch shapes: work items, the sites of one, the workgroups, and the bound on a workgroup's sites.
// The level array lives on the heap at its exact length, so a read past nlevels is the sanitizer's.
// Prints "OK <checks>" and returns 0, or every failure and 1.
#include <algorithm>
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
#define BFLBM_HIST_HOST_ONLY
#include "bflbm_hist.h"
#define BFLBM_MORPH_HOST_ONLY
#include "bflbm_morph.h"
#define BFLBM_CHORD_HOST_ONLY
#include "bflbm_chord.h"

typedef std::vector<double> Doubles;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static void expect_refusal(const char* want, int source, int var, int nlevels, const Doubles* levels, int side, int max_length) {
  g_msg.clear();
  const int rc = chord_refuse_args("X", source, var, nlevels, levels ? levels->data() : nullptr, side, max_length);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // ---- 1. accepted arguments and the layout ----------------------------------------------------------------------------
  const Doubles good = {0.25, 0.75};
  g_msg.clear();
  expect(chord_refuse_args("X", 0, 21, 2, good.data(), 1, 64) == 0 && g_msg.empty(), "good arguments pass");
  expect(chord_words(1) == 13 && chord_words(4) == 22 && chord_words(64) == 202 && chord_words(4096) == 12298, "W = 1 + 3 (3 + M)");
  expect(chord_block(64, 0) == 1 && chord_block(64, 1) == 68 && chord_block(64, 2) == 135 && chord_block(64, 2) + 3 + 64 == chord_words(64),
         "the axis blocks lie side by side after word 0");
  expect(chord_block(1, 0) == 1 && chord_block(1, 1) == 5 && chord_block(1, 2) == 9, "max_length 1: blocks of four words");

  // ---- 2. refusals: one bad argument each, the morphology trace's first ------------------------------------------------
  expect_refusal("X: 1..8 levels (got 0)", 0, 0, 0, &good, 0, 64);
  expect_refusal("X: 1..8 levels (got 9)", 0, 0, 9, &good, 0, 0);                      // before max_length
  expect_refusal("X: null argument", 0, 0, 2, nullptr, 0, 64);
  {
    const Doubles l_nan = {0.25, nan};
    expect_refusal("X: level 1 is not finite (got nan)", 0, 0, 2, &l_nan, 0, 64);
  }
  expect_refusal("X: side must be 0 (v >= level) or 1 (v < level) (got 2)", 0, 0, 2, &good, 2, 64);
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got 2)", 2, 0, 2, &good, 0, 64);
  expect_refusal("X: variable index 22 outside hydrovs (0..21)", 0, 22, 2, &good, 0, 0);   // before max_length
  expect_refusal("X: variable index 9 outside hydrovsbar (0..8)", 1, 9, 2, &good, 0, 64);
  expect_refusal("X: max_length in 1..4096 (got 0)", 0, 0, 2, &good, 0, 0);
  expect_refusal("X: max_length in 1..4096 (got -3)", 0, 0, 2, &good, 0, -3);
  expect_refusal("X: max_length in 1..4096 (got 4097)", 0, 0, 2, &good, 0, 4097);

  // ---- 3. the counter cap: nlevels W <= 16384 --------------------------------------------------------------------------
  expect(chord_limits::kMaxCounters == 16384 && chord_limits::kMaxLength == 4096, "the caps");
  expect(chord_refuse_args("X", 0, 0, 1, good.data(), 0, 4096) == 0, "one level of the longest record passes: 12298 counters");
  expect_refusal("X: 2 levels x 12298 words = 24596 counters per replica exceed 16384", 0, 0, 2, &good, 0, 4096);
  {
    const Doubles eight(8, 1.0);
    expect(8 * chord_words(679) == 16376 && chord_refuse_args("X", 1, 8, 8, eight.data(), 0, 679) == 0, "8 levels x 2047 words pass");
    expect_refusal("X: 8 levels x 2050 words = 16400 counters per replica exceed 16384", 0, 0, 8, &eight, 0, 680);
  }

  // ---- 4. the launch shapes ----------------------------------------------------------------------------------------------
  // (7, 9, 5): 45 rows in 12 items of 4; 35 lines (y) and 63 lines (z) in one item each
  expect(chord_items(0, 7, 9, 5) == 12 && chord_items(1, 7, 9, 5) == 1 && chord_items(2, 7, 9, 5) == 1, "(7, 9, 5): work items");
  expect(chord_item_sites(0, 7, 9, 5) == 28 && chord_item_sites(1, 7, 9, 5) == 35 * 9 && chord_item_sites(2, 7, 9, 5) == 63 * 5, "(7, 9, 5): sites of a work item");
  expect(chord_groups(0, 7, 9, 5, 1) == 12 && chord_groups(1, 7, 9, 5, 1) == 1 && chord_groups(2, 7, 9, 5, 3) == 1, "(7, 9, 5): a workgroup per work item");
  // (34, 31, 19): 646 y lines in 3 items, 1054 z lines in 5
  expect(chord_items(1, 34, 31, 19) == 3 && chord_items(2, 34, 31, 19) == 5 && chord_items(0, 34, 31, 19) == 148, "(34, 31, 19): work items");
  // an extent of 1: one row of one site is a work item of min(4, rows) sites
  expect(chord_item_sites(0, 1, 1, 1) == 1 && chord_groups(0, 1, 1, 1, 1) == 1 && chord_groups(2, 1, 1, 1, 1) == 1, "(1, 1, 1)");
  // 256^3: 16384 row items over 2048 workgroups: the launch strides; 256 march items, one workgroup each
  expect(chord_items(0, 256, 256, 256) == 16384 && chord_groups(0, 256, 256, 256, 1) == 2048, "256^3: the x launch strides over its work items");
  expect(chord_items(2, 256, 256, 256) == 256 && chord_groups(1, 256, 256, 256, 1) == 256 && chord_groups(2, 256, 256, 256, 1) == 256, "256^3: the marches");
  // 16 replicas of 64^3: 1024 row items over 128 workgroups per replica, 16 march items
  expect(chord_groups(0, 64, 64, 64, 16) == 128 && chord_groups(2, 64, 64, 64, 16) == 16, "16 x 64^3");
  expect(chord_groups(0, 8, 8, 8, 4096) == 1, "more replicas than workgroups wanted: one per replica");
  // the bound: 2048^3 has 2^20 row items of 8192 sites: 2048 workgroups would meet 2^32 / 2048 = 2^22 sites each, fine; a box of
  // 2^16 x 2^16 x 4 has 2^18 rows of 65536 sites, 2^16 items of 2^18 sites: 2048 groups meet 2^23 sites.  A plane of 2^30 sites
  // marched over 2^20 planes would meet 2^28 sites per item: four items per workgroup at the most
  expect(chord_item_sites(2, 1 << 15, 1 << 15, 1 << 20) == (1LL << 28) && chord_items(2, 1 << 15, 1 << 15, 1 << 20) == (1LL << 22)
             && chord_groups(2, 1 << 15, 1 << 15, 1 << 20, 1) == (1LL << 20),
         "no workgroup meets more than 2^30 sites");
  expect(chord_groups(1, 3, 1 << 22, 5, 1) == 1 && chord_item_sites(1, 3, 1 << 22, 5) == 15LL << 22, "a work item below 2^30 sites stays whole");

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
