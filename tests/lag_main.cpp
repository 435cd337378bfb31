// Stand-alone host check of the lag trace's host part (csrc/bflbm_lag.h under BFLBM_LAG_HOST_ONLY, on top of the host part
// of csrc/bflbm_fieldsel.h: no HIP, no library).  Built and run by tests/test_lag_abi.py with -fsanitize=address,undefined.
// It checks
//   1. the layout of a sample: W and the place of every word, against values written out by hand;
//   2. the slot schedule (which slot takes an origin, which slots are live) against a plain walk over the samples;
//   3. every refusal of the arguments, one bad argument each and in the header's order, the message compared in full;
//   4. the launch shape and the buffers of the boxes the GPU tests run and of the measured workloads.
// The argument arrays live on the heap at their exact length, so a read past nvars or npairs is the sanitizer's.
// Prints "OK <checks>" and returns 0, or every failure and 1.
#include <cmath>
#include <cstdarg>
#include <cstdio>
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
#define BFLBM_LAG_HOST_ONLY
#include "bflbm_lag.h"

typedef std::vector<int> Ints;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static int refuse(int source, const Ints& vars, const Ints& a, const Ints& b, int R, int E, int pslot, double level) {
  g_msg.clear();
  return lag_refuse_args("X", source, (int)vars.size(), vars.data(), (int)a.size(), a.data(), b.data(), R, E, pslot, level);
}

static void expect_refusal(const char* want, int source, const Ints& vars, const Ints& a, const Ints& b, int R, int E, int pslot, double level) {
  const int rc = refuse(source, vars, a, b, R, E, pslot, level);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // ---- 1. the layout -----------------------------------------------------------------------------------------------------
  expect(lag_words(1, 1, 1) == 4 && lag_words(3, 3, 8) == 43 && lag_words(4, 3, 8) == 44 && lag_words(8, 8, 16) == 168, "W = nvars + R (2 + npairs)");
  expect(lag_word_origin_step(3, 2, 0) == 3 && lag_word_alive(3, 2, 0) == 4 && lag_word_corr(3, 2, 0, 0) == 5 && lag_word_corr(3, 2, 0, 1) == 6
             && lag_word_origin_step(3, 2, 1) == 7 && lag_word_corr(3, 2, 2, 1) == 14 && lag_words(3, 2, 3) == 15,
         "now, then per slot the label, the count and the pairs");
  for (int nv = 1; nv <= 8; ++nv)
    for (int np = 1; np <= 8; ++np)
      expect(lag_word_corr(nv, np, 15, np - 1) == lag_words(nv, np, 16) - 1 && lag_word_origin_step(nv, np, 0) == nv, "the last word is the last pair of the last slot");

  // ---- 2. the slot schedule ----------------------------------------------------------------------------------------------
  {
    const int cases[4][3] = {{1, 1, 5}, {3, 2, 8}, {16, 1, 8}, {2, 3, 20}};           // R, E, samples
    for (const auto& c : cases) {
      const int R = c[0], E = c[1];
      unsigned live = 0u;
      int next = 0;                                          // the slot the next origin goes to
      bool same = true;
      for (int n = 0; n < c[2]; ++n) {
        int take = -1;
        if (n % E == 0) { take = next; live |= 1u << next; next = (next + 1) % R; }
        same = same && lag_take(n, R, E) == take && lag_live(n, R, E) == live;
      }
      expect(same, "take and live against a walk");
    }
    expect(lag_take(0, 16, 1) == 0 && lag_take(15, 16, 1) == 15 && lag_take(16, 16, 1) == 0 && lag_live(15, 16, 1) == 0xffffu && lag_live(1000, 16, 1) == 0xffffu,
           "16 slots wrap and stay live");
    expect(lag_take(7, 3, 2) == -1 && lag_take(6, 3, 2) == 0 && lag_live(3, 3, 2) == 3u && lag_live(4, 3, 2) == 7u, "R = 3, E = 2");
    expect(lag_take((1LL << 40) * 4, 8, 4) == 0 && lag_live(1LL << 40, 8, 4) == 0xffu, "the sample count is 64 bits");
  }

  // ---- 3. refusals: one bad argument each, in the header's order ---------------------------------------------------------
  const Ints v3 = {2, 3, 4}, a3 = {0, 1, 2}, b3 = {0, 1, 2};
  expect(refuse(0, v3, a3, b3, 8, 4, -1, nan) == 0 && g_msg.empty(), "three variables with themselves, no persistence: the level is not looked at");
  expect(refuse(1, {1, 2, 3, 4}, a3, {3, 3, 0}, 16, 1, 0, 1.0) == 0, "hydrovsbar, persistence of slot 0");
  expect(refuse(0, {0, 1, 2, 3, 4, 9, 12, 21}, {0, 1, 2, 3, 4, 5, 6, 7}, {7, 6, 5, 4, 3, 2, 1, 0}, 1, 1000, 7, -0.0) == 0, "the limits themselves");
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got 2)", 2, v3, a3, b3, 8, 1, -1, 0.);
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got -1)", -1, {}, {}, {}, 0, 0, -2, nan);      // before everything else
  expect_refusal("X: 1..8 variables (got 0)", 0, {}, {}, {}, 0, 0, -2, nan);
  expect_refusal("X: 1..8 variables (got 9)", 0, {0, 1, 2, 3, 4, 5, 6, 7, 8}, a3, b3, 8, 1, -1, 0.);
  expect_refusal("X: 1..8 pairs (got 0)", 0, v3, {}, {}, 8, 1, -1, 0.);
  expect_refusal("X: 1..8 pairs (got 9)", 0, v3, Ints(9, 0), Ints(9, 0), 8, 1, -1, 0.);
  expect_refusal("X: variable index 22 outside hydrovs (0..21)", 0, {0, 22}, {0}, {0}, 8, 1, -1, 0.);
  expect_refusal("X: variable index 9 outside hydrovsbar (0..8)", 1, {9}, {0}, {0}, 8, 1, -1, 0.);
  expect_refusal("X: variable index 3 given twice", 0, {3, 1, 3}, {0}, {0}, 8, 1, -1, 0.);
  expect_refusal("X: pair 1: slot 3 outside the 3 variables", 0, v3, {0, 3}, {0, 0}, 8, 1, -1, 0.);
  expect_refusal("X: pair 0: slot -1 outside the 3 variables", 0, v3, {0}, {-1}, 0, 0, -2, nan);                  // before R
  expect_refusal("X: 1..16 origins (got 0)", 0, v3, a3, b3, 0, 0, -2, nan);
  expect_refusal("X: 1..16 origins (got 17)", 0, v3, a3, b3, 17, 1, -1, 0.);
  expect_refusal("X: origin_stride must be >= 1 (got 0)", 0, v3, a3, b3, 16, 0, -2, nan);
  expect_refusal("X: persist_slot -2 outside -1..2", 0, v3, a3, b3, 16, 1, -2, nan);
  expect_refusal("X: persist_slot 3 outside -1..2", 0, v3, a3, b3, 16, 1, 3, 0.);
  expect_refusal("X: persist_level must be finite (got nan)", 0, v3, a3, b3, 16, 1, 0, nan);
  expect_refusal("X: persist_level must be finite (got inf)", 0, v3, a3, b3, 16, 1, 2, inf);
  expect_refusal("X: persist_level must be finite (got -inf)", 0, v3, a3, b3, 16, 1, 2, -inf);

  // ---- 4. the launch shape and the buffers -------------------------------------------------------------------------------
  expect(lag_limits::kTile == 2048 && lag_limits::kPerThread == 8 && lag_limits::kMaxOrigins == 16 && lag_limits::kMaxPairs == 8, "the limits");
  expect(lag_tiles(33 * 7) == 1 && lag_tiles(64 * 32) == 1 && lag_tiles(70 * 33) == 2 && lag_tiles(16 * 8) == 1 && lag_tiles(2049) == 2
             && lag_tiles(256 * 256) == 32 && lag_tiles(64 * 64) == 2 && lag_tiles(1LL << 31) == (1 << 20),
         "tiles of 2048 sites of a plane");
  expect(lag_qtot(1, 1, 1) == 2 && lag_qtot(3, 3, 8) == 27 && lag_qtot(4, 3, 8) == 28 && lag_qtot(8, 8, 16) == 136, "sums per (plane, tile)");
  // (70, 33, 4), 3 variables, 2 pairs, 3 origins: 9 sums on 4 planes of 2 tiles; 9240 sites
  expect(lag_origin_bytes(1, 3, 3, 9240) == 665280u && lag_mask_bytes(1, 9240, 0) == 18480u && lag_mask_bytes(1, 9240, -1) == 0u
             && lag_stage_partials(1, 4, 9, 2) == 72u && lag_stage_planes(1, 4, 9) == 36u && lag_stage_words(1, 4, 9, 2, 3) == 114u,
         "(70, 33, 4)");
  // 3 replicas of (16, 8, 8), 3 variables, 2 pairs, 3 origins: what tests/test_gpu_lag.py asks bflbm_lag_geometry for
  expect(lag_origin_bytes(3, 3, 3, 1024) == 221184u && lag_mask_bytes(3, 1024, 1) == 6144u && lag_stage_words(3, 8, 9, 1, 3) == 216u + 216u + 18u
             && lag_origin_bytes(1, 16, 3, 9240) == 3548160u && lag_words(3, 2, 3) == 15 && lag_words(3, 2, 16) == 67,
         "3 x (16, 8, 8), and (70, 33, 4) with 16 origins");
  // 256^3 with phi and three velocities, 8 origins: 4 GiB of origins, 32 MiB of masks
  expect(lag_origin_bytes(1, 8, 4, 1LL << 24) == (4ull << 30) && lag_mask_bytes(1, 1LL << 24, 0) == (32ull << 20)
             && lag_stage_partials(1, 256, 28, 32) == 229376u && lag_stage_words(1, 256, 28, 32, 8) == 229376u + 7168u + 16u,
         "256^3");
  // 16 replicas of 64^3, the same settings: 1 GiB of origins
  expect(lag_origin_bytes(16, 8, 4, 1LL << 18) == (1ull << 30) && lag_mask_bytes(16, 1LL << 18, 0) == (8ull << 20) && lag_stage_words(16, 64, 28, 2, 8) == 57344u + 28672u + 256u,
         "16 x 64^3");

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
