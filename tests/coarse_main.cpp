// Stand-alone host check of the coarse trace's host part (csrc/bflbm_coarse.h under BFLBM_COARSE_HOST_ONLY: no HIP, no
// library).  Built and run by tests/test_coarse_abi.py with -fsanitize=address,undefined.  It checks
//   1. accepted windows and blocks, the coarse cells c_a = w_a / b_a;
//   2. every refusal of the window and the block, one bad argument each and in the header's order, the message compared
//      in full;
//   3. the x-tile, the tiles of a row, the lanes of a work item and the work items a workgroup shares;
//   4. the work items and the workgroups of the boxes the GPU tests run, of the measured workloads and of the limits.
// The triples live on the heap at their exact length, so a read past three entries is the sanitizer's.
// Prints "OK <checks>" and returns 0, or every failure and 1.
#include <algorithm>
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

#define BFLBM_COARSE_HOST_ONLY
#include "bflbm_coarse.h"

typedef std::vector<int> Ints;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static int refuse(const Ints& n, const Ints& o, const Ints& w, const Ints& b) {
  g_msg.clear();
  return coarse_refuse_window("X", n.data(), o.data(), w.data(), b.data());
}

static void expect_refusal(const char* want, const Ints& n, const Ints& o, const Ints& w, const Ints& b) {
  const int rc = refuse(n, o, w, b);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

// (c_x, c_y, c_z, tile, ntiles, lanes, share, items) of an accepted window
static bool shape_is(const Ints& n, const Ints& o, const Ints& w, const Ints& b, int cx, int cy, int cz, int tile, int ntiles, int lanes,
                     int share, int items) {
  if (refuse(n, o, w, b) != 0) return false;
  const CoarseGeo g = coarse_geo(n.data(), o.data(), w.data(), b.data());
  bool same = true;
  for (int a = 0; a < 3; ++a) same = same && g.n[a] == n[a] && g.o[a] == o[a] && g.w[a] == w[a] && g.b[a] == b[a];
  return same && g.c[0] == cx && g.c[1] == cy && g.c[2] == cz && g.tile == tile && g.ntiles == ntiles && g.lanes == lanes && g.share == share
         && g.items == items && coarse_items(w.data(), b.data()) == items;
}

int main() {
  const Ints box = {10, 6, 13}, zero = {0, 0, 0}, one = {1, 1, 1};
  // ---- 1. accepted arguments ---------------------------------------------------------------------------------------------
  expect(refuse(box, zero, box, one) == 0 && g_msg.empty(), "the full window at block 1 passes");
  expect(refuse(box, {9, 5, 12}, box, {10, 6, 13}) == 0, "the last site as origin, the full extent, one block");
  expect(refuse(box, {8, 5, 11}, {6, 4, 6}, {3, 2, 3}) == 0, "a window through the seam on all three axes");
  expect(refuse({512, 2, 2}, zero, {512, 2, 2}, {256, 2, 1}) == 0, "b_x = 256 passes");

  // ---- 2. refusals: one bad argument each, in the header's order -----------------------------------------------------------
  expect_refusal("X: origin[x] = -1 outside 0..9", box, {-1, 0, 0}, box, one);
  expect_refusal("X: origin[x] = 10 outside 0..9", box, {10, 0, 0}, box, one);
  expect_refusal("X: origin[y] = 6 outside 0..5", box, {0, 6, 0}, box, one);
  expect_refusal("X: origin[z] = 13 outside 0..12", box, {0, 0, 13}, {0, 0, 0}, zero);       // before the extent and the block
  expect_refusal("X: extent[x] = 0 outside 1..10", box, zero, {0, 6, 13}, zero);              // before the block
  expect_refusal("X: extent[x] = 11 outside 1..10", box, zero, {11, 6, 13}, one);
  expect_refusal("X: extent[y] = 7 outside 1..6", box, zero, {10, 7, 13}, one);
  expect_refusal("X: extent[z] = -2 outside 1..13", box, zero, {10, 6, -2}, one);
  expect_refusal("X: block[x] must be >= 1 (got 0)", box, zero, box, {0, 1, 1});
  expect_refusal("X: block[y] must be >= 1 (got -3)", box, zero, box, {1, -3, 1});
  expect_refusal("X: block[x] = 3 does not divide the extent 10", box, zero, box, {3, 1, 1});
  expect_refusal("X: block[y] = 4 does not divide the extent 6", box, zero, box, {5, 4, 1});
  expect_refusal("X: block[z] = 2 does not divide the extent 13", box, zero, box, {5, 3, 2});
  expect_refusal("X: block[z] = 5 does not divide the extent 6", box, {8, 5, 11}, {6, 4, 6}, {3, 2, 5});
  expect_refusal("X: block[x] = 257 exceeds 256", {514, 2, 2}, zero, {514, 2, 2}, {257, 1, 1});
  expect_refusal("X: block[y] must be >= 1 (got 0)", {514, 2, 2}, zero, {514, 2, 2}, {257, 0, 1});           // b_y before b_x > 256

  // ---- 3. the tile and the lanes -------------------------------------------------------------------------------------------
  expect(coarse_tile(1) == 256 && coarse_tile(2) == 256 && coarse_tile(3) == 255 && coarse_tile(65) == 195 && coarse_tile(128) == 256
             && coarse_tile(129) == 129 && coarse_tile(255) == 255 && coarse_tile(256) == 256,
         "an x-tile is floor(256 / b_x) b_x sites");
  for (int bx = 1; bx <= 256; ++bx) {
    const int t = coarse_tile(bx);
    expect(t % bx == 0 && t <= 256 && t + bx > 256, "whole blocks, within a workgroup, as many as fit");
  }
  expect(coarse_tiles(258, 3) == 2 && coarse_tiles(255, 3) == 1 && coarse_tiles(520, 1) == 3 && coarse_tiles(512, 256) == 2 && coarse_tiles(1, 1) == 1,
         "the tiles of a window row");
  expect(coarse_lanes(8, 2) == 64 && coarse_lanes(64, 2) == 64 && coarse_lanes(65, 1) == 128 && coarse_lanes(70, 7) == 128
             && coarse_lanes(130, 1) == 192 && coarse_lanes(260, 65) == 256 && coarse_lanes(4096, 1) == 256,
         "the lanes of a work item: whole waves");

  // ---- 4. the launch shapes ------------------------------------------------------------------------------------------------
  expect(shape_is({8, 8, 8}, zero, {8, 8, 8}, {2, 2, 2}, 4, 4, 4, 256, 1, 64, 4, 16), "(8, 8, 8) at 2 x 2 x 2");
  expect(shape_is(box, {0, 0, 1}, {10, 6, 12}, {5, 3, 4}, 2, 2, 3, 255, 1, 64, 4, 6), "(10, 6, 13): a z offset, block 5 x 3 x 4");
  expect(shape_is(box, {8, 5, 11}, {6, 4, 6}, {3, 2, 3}, 2, 2, 2, 255, 1, 64, 4, 4), "(10, 6, 13): the seam");
  expect(shape_is(box, {0, 0, 5}, {10, 6, 1}, one, 10, 6, 1, 256, 1, 64, 4, 6), "(10, 6, 13): a slice");
  expect(shape_is({70, 9, 16}, zero, {70, 9, 16}, {7, 3, 2}, 10, 3, 8, 252, 1, 128, 2, 24), "(70, 9, 16): two waves per work item");
  expect(shape_is({258, 4, 2}, zero, {258, 4, 2}, {3, 1, 1}, 86, 4, 2, 255, 2, 256, 1, 16), "(258, 4, 2): the second tile holds one block");
  expect(shape_is({260, 3, 2}, zero, {260, 3, 2}, {65, 1, 1}, 4, 3, 2, 195, 2, 256, 1, 12), "(260, 3, 2): a tile of 195 sites");
  expect(shape_is({520, 2, 2}, zero, {520, 2, 2}, one, 520, 2, 2, 256, 3, 256, 1, 12), "(520, 2, 2): three tiles");
  expect(shape_is({512, 2, 2}, zero, {512, 2, 2}, {256, 2, 1}, 2, 1, 2, 256, 2, 256, 1, 4), "(512, 2, 2): the largest b_x");
  expect(coarse_groups(16, 4, 1) == 4 && coarse_groups(6, 4, 1) == 2 && coarse_groups(6, 4, 3) == 2 && coarse_groups(24, 2, 1) == 12
             && coarse_groups(1, 4, 1) == 1,
         "a workgroup per turn of `share` work items");
  // 256^3 at 4^3: 4096 work items, one per turn, over 2048 workgroups; one z slice at block 1: 256 work items
  expect(shape_is({256, 256, 256}, zero, {256, 256, 256}, {4, 4, 4}, 64, 64, 64, 256, 1, 256, 1, 4096) && coarse_groups(4096, 1, 1) == 2048,
         "256^3 at 4 x 4 x 4: the launch strides over its turns");
  expect(shape_is({256, 256, 256}, {0, 0, 128}, {256, 256, 1}, one, 256, 256, 1, 256, 1, 256, 1, 256) && coarse_groups(256, 1, 1) == 256,
         "256^3: a slice");
  // 16 replicas of 64^3 at 2^3: 1024 work items, four per turn, 128 workgroups per replica
  expect(shape_is({64, 64, 64}, zero, {64, 64, 64}, {2, 2, 2}, 32, 32, 32, 256, 1, 64, 4, 1024) && coarse_groups(1024, 4, 16) == 128,
         "16 x 64^3 at 2 x 2 x 2");
  expect(coarse_groups(16, 4, 4096) == 1, "more replicas than workgroups wanted: one per replica");
  // the cap: 2048^3 at block 1 has 2^22 rows of 8 tiles = 2^25 work items; 32768 x 32768 x 8192 at block 1 reaches 2^35
  {
    const Ints big = {2048, 2048, 2048}, wide = {32768, 32768, 8192};
    expect(coarse_items(big.data(), one.data()) == (1LL << 25) && coarse_items(wide.data(), one.data()) == (1LL << 30) * 32
               && coarse_limits::kMaxItems == (1LL << 30),
           "the work items are counted in 64 bits; the cap is 2^30");
    const Ints o = {0, 0, 0};
    expect(coarse_geo(wide.data(), o.data(), wide.data(), one.data()).items == (1 << 30), "a count past the cap is clamped, never wrapped");
  }

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
