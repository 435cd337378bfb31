// Stand-alone host check of the histogram trace's host part (csrc/bflbm_hist.h under BFLBM_HIST_HOST_ONLY, on top of the
// host part of csrc/bflbm_fieldsel.h: no HIP, no library).  Built and run by tests/test_hist_abi.py with
// -fsanitize=address,undefined.  It checks
//   1. the block layout (offsets, lengths, C) and the scales of accepted arguments, against values written out by hand;
//   2. every refusal of the arguments, one bad argument each, the message compared in full;
//   3. the launch shape: the LDS size class and the workgroups per replica.
// The argument arrays live on the heap at their exact length, so a read past nvars or npairs is the sanitizer's.
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
#define BFLBM_HIST_HOST_ONLY
#include "bflbm_hist.h"

typedef std::vector<int> Ints;
typedef std::vector<double> Doubles;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static void expect_refusal(const char* want, int source, const Ints& vars, const Doubles* lo, const Doubles* hi, const Ints* nbins,
                           int npairs, const Ints* a, const Ints* b) {
  g_msg.clear();
  const int rc = hist_refuse_args("X", source, (int)vars.size(), vars.data(), lo ? lo->data() : nullptr, hi ? hi->data() : nullptr,
                                  nbins ? nbins->data() : nullptr, npairs, a ? a->data() : nullptr, b ? b->data() : nullptr);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // ---- 1. the layout ---------------------------------------------------------------------------------------------------
  {
    // three variables of 4, 1 and 10 bins; the pairs (2, 0) and (0, 1): blocks of 7, 4, 13, 41, 5 counters
    const Ints vars = {3, 1, 21}, nb = {4, 1, 10}, pa = {2, 0}, pb = {0, 1};
    const Doubles lo = {0.0, -1.0, 1e-3}, hi = {1.0, 1.0, 3e-3};
    g_msg.clear();
    expect(hist_refuse_args("X", 0, 3, vars.data(), lo.data(), hi.data(), nb.data(), 2, pa.data(), pb.data()) == 0 && g_msg.empty(), "good arguments pass");
    const HistLayout L = hist_layout(3, lo.data(), hi.data(), nb.data(), 2, pa.data(), pb.data());
    expect(L.nvars == 3 && L.npairs == 2 && L.C == 70, "C of three variables and two pairs");
    const int off[5] = {0, 7, 11, 24, 65}, len[5] = {7, 4, 13, 41, 5};
    for (int k = 0; k < 5; ++k) expect(hist_block_offset(L, k) == off[k] && hist_block_length(L, k) == len[k], "block offsets and lengths");
    expect(L.scale[0] == 4.0 && L.scale[1] == 0.5 && L.scale[2] == 10.0 / (3e-3 - 1e-3), "scales: one division each");
    expect(L.lo[0] == 0.0 && L.lo[1] == -1.0 && L.lo[2] == 1e-3, "lo");
    expect(L.pa[0] == 2 && L.pb[0] == 0 && L.pa[1] == 0 && L.pb[1] == 1 && L.pa[2] == 0 && L.pb[3] == 0, "pair slots, the unused ones 0");
    expect(L.nbins[3] == 1 && L.scale[7] == 1.0 && L.voff[3] == 24 && L.poff[2] == 70, "the unused entries");
    // the tables the kernel forms a cell from: pair (2, 0) = bin_2 x 4 + bin_0, pair (0, 1) = bin_0 x 1 + bin_1
    expect(L.pmul[0][2] == 4 && L.pmul[0][0] == 1 && L.pmul[0][1] == 0 && L.pmul[1][0] == 1 && L.pmul[1][1] == 1 && L.pmul[1][2] == 0 &&
           L.pmul[2][0] == 0 && L.pmul[0][3] == 0, "cell multipliers");
    expect(L.vpairs[0] == 3 && L.vpairs[1] == 2 && L.vpairs[2] == 1 && L.vpairs[3] == 0 && L.pout[0] == 64 && L.pout[1] == 69 && L.pout[2] == 0,
           "the pairs of a slot and the outside counters");
  }
  {
    // the limits themselves: 8 variables, 4096 bins, a pair block that fills C to 16384 exactly
    const Ints one = {0}, most = {4096};
    const Doubles lo = {-1.0}, hi = {1.0};
    g_msg.clear();
    expect(hist_refuse_args("X", 2, 1, one.data(), lo.data(), hi.data(), most.data(), 0, nullptr, nullptr) == 0, "4096 bins of a noise moment pass");
    const HistLayout L = hist_layout(1, lo.data(), hi.data(), most.data(), 0, nullptr, nullptr);
    expect(L.C == 4099 && hist_lds_counters(L.C) == 16384 && hist_lds_counters(4096) == 4096, "LDS size classes");
    // two variables of 127 and 126 bins and their pair: 130 + 129 + (16002 + 1) = 16262 <= 16384; 127 x 127: 16390
    const Ints two = {0, 1}, nb = {127, 126}, pa = {0}, pb = {1};
    const Doubles lo2 = {0.0, 0.0}, hi2 = {1.0, 1.0};
    expect(hist_refuse_args("X", 1, 2, two.data(), lo2.data(), hi2.data(), nb.data(), 1, pa.data(), pb.data()) == 0, "16262 counters pass");
    expect(hist_layout(2, lo2.data(), hi2.data(), nb.data(), 1, pa.data(), pb.data()).C == 16262, "C = 130 + 129 + 16003");
    const Ints nb2 = {127, 127};
    expect_refusal("X: 16390 counters per replica exceed 16384", 1, two, &lo2, &hi2, &nb2, 1, &pa, &pb);
  }

  // ---- 2. refusals: one bad argument each ------------------------------------------------------------------------------
  const Ints good = {3, 1}, nb = {8, 16}, pa = {0}, pb = {1};
  const Doubles lo = {0.0, -2.0}, hi = {1.0, 2.0};
  expect_refusal("X: source must be 0 (hydrovs), 1 (hydrovsbar) or 2 (noise) (got 3)", 3, good, &lo, &hi, &nb, 0, nullptr, nullptr);
  expect_refusal("X: 1..8 variables (got 0)", 0, Ints(), &lo, &hi, &nb, 0, nullptr, nullptr);
  {
    const Ints nine = {0, 1, 2, 3, 4, 5, 6, 7, 8}, nb9(9, 4);
    const Doubles lo9(9, 0.0), hi9(9, 1.0);
    expect_refusal("X: 1..8 variables (got 9)", 0, nine, &lo9, &hi9, &nb9, 0, nullptr, nullptr);
  }
  expect_refusal("X: variable index 22 outside hydrovs (0..21)", 0, {3, 22}, &lo, &hi, &nb, 0, nullptr, nullptr);
  expect_refusal("X: variable index 38 outside the noise moments (0..37)", 2, {38, 0}, &lo, &hi, &nb, 0, nullptr, nullptr);
  expect_refusal("X: variable index 3 given twice", 0, {3, 3}, &lo, &hi, &nb, 0, nullptr, nullptr);
  expect_refusal("X: 0..4 pairs (got 5)", 0, good, &lo, &hi, &nb, 5, &pa, &pb);
  expect_refusal("X: 0..4 pairs (got -1)", 0, good, &lo, &hi, &nb, -1, &pa, &pb);
  expect_refusal("X: null argument", 0, good, &lo, &hi, &nb, 1, nullptr, &pb);
  expect_refusal("X: null argument", 0, good, nullptr, &hi, &nb, 0, nullptr, nullptr);
  expect_refusal("X: null argument", 0, good, &lo, nullptr, &nb, 0, nullptr, nullptr);
  expect_refusal("X: null argument", 0, good, &lo, &hi, nullptr, 0, nullptr, nullptr);
  {
    const Ints a = {2}, b = {0}, c = {1}, d = {1};
    expect_refusal("X: pair 0: slot 2 outside the 2 variables", 0, good, &lo, &hi, &nb, 1, &a, &b);
    expect_refusal("X: pair 0: slot 1 with itself", 0, good, &lo, &hi, &nb, 1, &c, &d);
  }
  {
    const Doubles lo_nan = {0.0, nan}, hi_inf = {1.0, inf}, lo_minf = {-inf, -2.0}, hi_eq = {1.0, -2.0}, hi_less = {-1.0, 2.0};
    expect_refusal("X: variable slot 1: the range needs finite lo < hi (got nan, 2)", 0, good, &lo_nan, &hi, &nb, 0, nullptr, nullptr);
    expect_refusal("X: variable slot 1: the range needs finite lo < hi (got -2, inf)", 0, good, &lo, &hi_inf, &nb, 0, nullptr, nullptr);
    expect_refusal("X: variable slot 0: the range needs finite lo < hi (got -inf, 1)", 0, good, &lo_minf, &hi, &nb, 0, nullptr, nullptr);
    expect_refusal("X: variable slot 1: the range needs finite lo < hi (got -2, -2)", 0, good, &lo, &hi_eq, &nb, 0, nullptr, nullptr);
    expect_refusal("X: variable slot 0: the range needs finite lo < hi (got 0, -1)", 0, good, &lo, &hi_less, &nb, 0, nullptr, nullptr);
  }
  {
    const Ints zero = {8, 0}, many = {4097, 16};
    expect_refusal("X: variable slot 1: 1..4096 bins (got 0)", 0, good, &lo, &hi, &zero, 0, nullptr, nullptr);
    expect_refusal("X: variable slot 0: 1..4096 bins (got 4097)", 0, good, &lo, &hi, &many, 0, nullptr, nullptr);
  }
  {
    // hi - lo overflows: the scale is 0; hi - lo is the smallest subnormal: the scale is inf
    const double big = std::numeric_limits<double>::max(), tiny = std::numeric_limits<double>::denorm_min();
    const Doubles lo_big = {-big, -2.0}, hi_big = {big, 2.0}, lo_0 = {0.0, -2.0}, hi_tiny = {tiny, 2.0};
    expect_refusal("X: variable slot 0: the scale nbins / (hi - lo) = 0 is not finite and positive", 0, good, &lo_big, &hi_big, &nb, 0, nullptr, nullptr);
    expect_refusal("X: variable slot 0: the scale nbins / (hi - lo) = inf is not finite and positive", 0, good, &lo_0, &hi_tiny, &nb, 0, nullptr, nullptr);
  }

  // ---- 3. the launch shape ---------------------------------------------------------------------------------------------
  expect(hist_tiles(1) == 1 && hist_tiles(2048) == 1 && hist_tiles(2049) == 2, "tiles of 2048 sites");
  expect(hist_groups(315, 1) == 1 && hist_groups(2049, 1) == 2 && hist_groups(2049, 3) == 2, "small boxes: one workgroup per tile");
  expect(hist_groups(1LL << 24, 1) == 512 && hist_groups(1LL << 18, 16) == 32 && hist_groups(1LL << 18, 1000) == 1, "512 workgroups over the replicas");
  expect(hist_groups(1056768, 1) == 512 && hist_tiles(1056768) == 516, "a box whose workgroups take a second tile");
  // 2^42 sites: 2^31 tiles, 2^20 per workgroup at the most, so that no workgroup meets 2^31 sites
  expect(hist_groups(1LL << 42, 1) == 2048 && hist_groups((1LL << 42) + 1, 1) == 2049, "the groups that keep a 32-bit counter from wrapping");

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
